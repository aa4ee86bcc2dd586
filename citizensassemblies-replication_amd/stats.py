"""Consumers of the LEGACY results.

* ``compute_prob_allocation_stats`` / ``upper_confidence_bound``: analysis.py:231-268,
  same arithmetic (the Gini sum in sorted order, scipy's gmean and beta.ppf), host side:
  they read n numbers.
* ``sorted_pair_probabilities``: the curve ``plot_pair_probability_distribution_per_algorithm``
  draws (analysis.py:339-342: ``sorted(histogram.get_dict().values())``, n(n-1)/2 values,
  33.5 M at n = 8192).  For a LEGACY histogram the pair counts are integers <= S, so the
  sorted list is a histogram of the counts: ``pair_histogram_kernel`` bins the upper
  triangle on the device and the host expands ``v / S`` (float64 true division, as the
  reference) ``hist[v]`` times.  A LEXIMIN / XMIN portfolio histogram built by
  ``analysis.portfolio_probabilities`` whose float64 triangle is still on the device is sorted
  there (``torch.sort``) and copied once; other float histograms (uniform, host-built) are
  sorted on the host.
"""
import contextlib
import ctypes
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import _native as N


@dataclass
class ProbAllocationStats:
    """analysis.py:61-65."""
    gini: float
    geometric_mean: float
    min: float


def compute_prob_allocation_stats(alloc, cap_for_geometric_mean: bool) -> ProbAllocationStats:
    """analysis.py:231-255 (same summation order, so the same floats)."""
    from scipy.stats import gmean
    n = len(alloc)
    k = round(sum(alloc.values()))
    sorted_probs = sorted(alloc.values())
    gini = sum((2 * i - n + 1) * prob for i, prob in enumerate(sorted_probs)) / (n * k)
    if cap_for_geometric_mean:
        geometric_mean = gmean([max(prob, 1 / 10000) for prob in alloc.values()])
    else:
        geometric_mean = gmean(sorted_probs)
    return ProbAllocationStats(gini=gini, geometric_mean=geometric_mean, min=min(sorted_probs))


def upper_confidence_bound(num_trials: int, sample_proportion: float) -> float:
    """analysis.py:258-268: 99th percentile of the Jeffreys posterior."""
    from scipy.stats import beta
    num_successes = round(sample_proportion * num_trials)
    if num_successes == num_trials:
        return 1.
    return beta.ppf(.99, .5 + num_successes, .5 + num_trials - num_successes)


def pair_count_histogram(d_pairs, n, n_bins, stream=None):
    """hist[v] = number of pairs i < j with count v, from device pair counts (torch int64,
    n*n row-major) via pair_histogram_kernel.  Returns a host uint64 array of n_bins."""
    import torch
    dev = d_pairs.device
    hist = torch.empty(int(n_bins), dtype=torch.int64, device=dev)
    over = torch.empty(1, dtype=torch.int64, device=dev)
    st = stream or torch.cuda.current_stream(dev)
    N.check(N.lib().csa_pair_histogram_async(N.ptr(d_pairs), int(n), N.ptr(hist), int(n_bins), N.ptr(over),
                                             ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    if int(over.item()):
        raise ValueError("pair counts exceed n_bins = %d" % n_bins)
    return hist.cpu().numpy().view(np.uint64)


def sorted_counts_to_probabilities(hist, S):
    v = np.flatnonzero(hist)
    return np.repeat(v.astype(np.int64) / S, hist[v].astype(np.int64))


def sorted_pair_probabilities(pair_histogram, device="cuda"):
    """Ascending list of all pair values of a PairHistogram (analysis.py:339-342), as float64."""
    counts, S = getattr(pair_histogram, "_counts", None), getattr(pair_histogram, "_S", None)
    if counts is None or S is None:
        tri = getattr(pair_histogram, "_dtri", None)
        if tri is not None and pair_histogram._uv is None and not pair_histogram._divs:
            # a LEXIMIN / XMIN portfolio histogram whose triangle is still on the device
            # (analysis.portfolio_probabilities): sorted there, one copy of the sorted values
            import torch
            m = len(pair_histogram)
            return torch.sort(tri[:m]).values.cpu().numpy()
        return np.sort(pair_histogram.upper())      # any other float histogram: sorted on the host
    import torch
    n = counts.shape[0]
    if isinstance(counts, np.ndarray):
        d = torch.from_numpy(np.ascontiguousarray(counts, np.int64)).to(device)
    else:
        d = counts.reshape(n, n)              # device counts kept by legacy_probabilities: no host copy
    # every pair count is <= both person counts (the diagonal); the max over the triangle covers
    # matrices whose diagonal was not kept as well
    n_bins = int(torch.triu(d).max().item()) + 1 if n else 1
    return sorted_counts_to_probabilities(pair_count_histogram(d.contiguous().view(-1), n, n_bins), S)


# ---- group composition: what a panel looks like as a whole ----------------------------------------
#
# A group is a set of agents held as a uint64[W] bitmask in encoding order (agent p = bit p & 63 of
# word p >> 6, padding bits zero): a quota feature, a two-feature intersection
# (plot_intersectional_representation, analysis.py:459-530), a household.  ``group_composition``
# counts, per group, the panels that hold 0, 1, ..., k of its members -- group_hist_kernel
# (csrc/composition.inc) on the device, the numpy implementation below without one.  For a LEXIMIN /
# XMIN portfolio, whose panels carry probabilities, ``portfolio_group_composition`` further down.

class GroupSet:
    """``labels`` (list), ``masks`` uint64[G, W], ``sizes`` int64[G] (members per group).  ``a + b``
    concatenates two sets over the same encoding."""

    def __init__(self, labels, masks, sizes=None):
        self.labels = list(labels)
        m = np.ascontiguousarray(masks, np.uint64)
        assert m.ndim == 2 and m.shape[0] == len(self.labels)
        self.masks = m
        self.sizes = _popcount_rows(m) if sizes is None else np.asarray(sizes, np.int64)

    @property
    def W(self):
        return self.masks.shape[1]

    def __len__(self):
        return len(self.labels)

    def check_width(self, W):
        """ValueError unless the masks have the W words of the encoding they are used with."""
        if self.W != W:
            raise ValueError("groups of another encoding: W = %d, the instance has %d" % (self.W, W))

    def device_masks(self, device, W=None):
        """The masks as G*W int64 words on ``device`` (a blocking upload on the current stream), for
        panels of ``W`` words when given: ValueError for groups of another encoding."""
        import torch
        if W is not None:
            self.check_width(W)
        return torch.from_numpy(self.masks.view(np.int64).reshape(-1)).to(device)

    def __add__(self, other):
        if not isinstance(other, GroupSet):
            return NotImplemented
        if other.W != self.W:
            raise ValueError("group sets of different encodings: W = %d and %d" % (self.W, other.W))
        return GroupSet(self.labels + other.labels, np.concatenate([self.masks, other.masks]),
                        np.concatenate([self.sizes, other.sizes]))


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _popcount_rows(words):
    """Set bits per row of a uint64[R, W] array."""
    w = np.ascontiguousarray(words, np.uint64)
    return _POP8[w.view(np.uint8).reshape(w.shape[0], -1)].sum(axis=1)


def _pack_members(member, W):
    """bool[G, n] membership -> uint64[G, W] masks (padding bits zero)."""
    G, n = member.shape
    x = np.zeros((G, max(W, 1) * 64), np.bool_)
    x[:, :n] = member
    return np.ascontiguousarray(np.packbits(x, axis=1, bitorder="little")).view("<u8").reshape(G, max(W, 1))


def _encoding(instance):
    from .instance import encode_cached
    return encode_cached(instance.categories, instance.agents)


def _feature_membership(enc):
    """bool[F, n]: agent p holds feature f (each agent one feature per category)."""
    member = np.zeros((enc.F, enc.n), np.bool_)
    if enc.n:
        for c in range(enc.C):
            member[enc.person_feat[:, c], np.arange(enc.n)] = True
    return member


def feature_groups(instance):
    """One group per (category, feature), in ``EncodedInstance.feat_keys`` order."""
    enc = _encoding(instance)
    member = _feature_membership(enc)
    return GroupSet(list(enc.feat_keys), _pack_members(member, enc.W), member.sum(axis=1))


def read_intersections(path):
    """Rows of an ``intersections.csv``-shaped table as ((c1, f1), (c2, f2), population share)."""
    import csv
    rows = []
    with open(path, "r", encoding="utf-8") as fh:
        for entry in csv.DictReader(fh):
            rows.append(((entry["category 1"], entry["feature 1"]), (entry["category 2"], entry["feature 2"]),
                         float(entry["population share"])))
    return rows


def _intersection_rows(rows):
    import os
    if isinstance(rows, (str, os.PathLike)):
        return [(a, b) for a, b, _ in read_intersections(rows)]
    return [(tuple(r[0]), tuple(r[1])) for r in rows]


def _feature_index(enc):
    """(category, feature) -> feature id; KeyError on an unknown category or feature."""
    fid = {key: f for f, key in enumerate(enc.feat_keys)}
    cats = set(enc.cat_names)

    def index(key):
        key = tuple(key)
        if key[0] not in cats or key not in fid:
            raise KeyError(key[0] if key[0] not in cats else key[1])
        return fid[key]
    return index


def intersection_groups(instance, rows):
    """One group per two-feature intersection: ``rows`` is a path to an ``intersections.csv``-shaped
    table or an iterable of ``((c1, f1), (c2, f2))``; the mask is the AND of the two feature masks
    (has_features, analysis.py:459-463).  Empty groups are kept; an unknown category or feature
    raises KeyError."""
    enc = _encoding(instance)
    index = _feature_index(enc)
    pairs = _intersection_rows(rows)
    member = _feature_membership(enc)
    both = np.zeros((len(pairs), enc.n), np.bool_)
    for g, (a, b) in enumerate(pairs):
        both[g] = member[index(a)] & member[index(b)]
    return GroupSet(pairs, _pack_members(both, enc.W), both.sum(axis=1))


def agent_groups(instance, groups):
    """Arbitrary agent sets ``{label: agent ids}`` (the rings of ``legacy.address_rings``, households);
    an id that is not in the instance raises KeyError."""
    enc = _encoding(instance)
    pos = {aid: p for p, aid in enumerate(enc.agent_ids)}
    labels = list(groups)
    member = np.zeros((len(labels), enc.n), np.bool_)
    for g, label in enumerate(labels):
        for aid in groups[label]:
            member[g, pos[aid]] = True
    return GroupSet(labels, _pack_members(member, enc.W), member.sum(axis=1))


def household_groups(agent_ids, columns_data, check_same_address_columns):
    """One group per household of at least two agents: the rings of ``legacy.address_rings`` over
    ``agent_ids`` (an encoding's ``agent_ids``), labelled by their (address, zip) values, in order of each
    household's first agent.  A household-aware run's ``legacy_composition`` over it shows no panel that
    holds two members of a household: every count at 2 or above is zero."""
    c0, c1 = check_same_address_columns[0], check_same_address_columns[1]
    homes = {}
    for p, aid in enumerate(agent_ids):
        row = columns_data[aid]
        homes.setdefault((row[c0], row[c1]), []).append(p)
    labels = [key for key, members in homes.items() if len(members) >= 2]
    n = len(agent_ids)
    member = np.zeros((len(labels), n), np.bool_)
    for g, key in enumerate(labels):
        member[g, homes[key]] = True
    return GroupSet(labels, _pack_members(member, (n + 63) // 64), member.sum(axis=1))


def group_hist_host(masks, panels, bins):
    """csa_group_hist_async's contract in numpy: int64[G, bins], hist[g][c] = number of panels with
    popcount(panel & mask_g) == c.  A count >= bins raises CsaError(CSA_E_INVALID), as the device's
    status block does.  The counts are a 0/1 matrix product (float32 sums of at most 64 W ones: exact)."""
    masks = np.ascontiguousarray(masks, np.uint64)
    panels = np.ascontiguousarray(panels, np.uint64)
    G, W = masks.shape
    S = panels.shape[0]
    assert panels.ndim == 2 and (S == 0 or panels.shape[1] == W)
    bins = int(bins)
    hist = np.zeros((G, bins), np.int64)
    if G == 0 or S == 0:
        return hist
    assert 64 * W < 1 << 24
    m = np.unpackbits(masks.view(np.uint8).reshape(G, -1), axis=1, bitorder="little").astype(np.float32)
    base = np.arange(G, dtype=np.int64) * bins
    step = max(1, (1 << 24) // (64 * W))
    for off in range(0, S, step):
        x = np.unpackbits(panels[off:off + step].view(np.uint8).reshape(-1, 8 * W), axis=1, bitorder="little")
        c = (x.astype(np.float32) @ m.T).astype(np.int64)                   # [panels, G]
        bad = np.argwhere(c >= bins)
        if len(bad):
            raise N.CsaError(N.CSA_E_INVALID, "group hist: panel %d holds %d members of group %d, bins = %d"
                             % (off + bad[0][0], c[bad[0][0], bad[0][1]], bad[0][1], bins))
        hist += np.bincount((c + base).ravel(), minlength=G * bins).reshape(G, bins)
    return hist


class _Composition:
    """What both composition tables derive: a subclass names its table (``_table``, [G, k + 1]) and
    the number it is normalised by (``_norm``), the instance attributes stay its own.  The bin index
    takes the table's dtype (int64 for counts, float64 for weights), so integer sums stay exact."""

    def __len__(self):
        return len(self.labels)

    def probabilities(self):
        """P(a panel holds c members), float64[G, k+1] = table / norm."""
        return self._table / self._norm

    def mean(self):
        """Expected members per panel (by linearity also the sum of the members' marginals)."""
        return (self._table * np.arange(self.k + 1, dtype=self._table.dtype)).sum(axis=1) / self._norm

    def panel_share(self):
        """mean / k: the panel share plot_intersectional_representation reports."""
        return self.mean() / self.k

    def variance(self):
        """Variance of the members per panel (population form: the table is the distribution)."""
        d = np.arange(self.k + 1, dtype=np.float64)[None, :] - self.mean()[:, None]
        return (self._table * d * d).sum(axis=1) / self._norm

    def prob_absent(self):
        """P(a panel holds no member of the group)."""
        return self._table[:, 0] / self._norm

    def support(self):
        """(lowest, highest) non-empty bin per group, int64[G] each; (-1, -1) where there is none."""
        nz = self._table != 0
        some = nz.any(axis=1)
        lo = np.where(some, nz.argmax(axis=1), -1)
        hi = np.where(some, self.k - nz[:, ::-1].argmax(axis=1), -1)
        return lo.astype(np.int64), hi.astype(np.int64)


class CompositionHistogram(_Composition):
    """``counts[g][c]`` = panels of the run holding exactly c members of group g (host int64[G, k+1]),
    over ``S`` panels of size ``k``; ``labels`` name the groups.  Everything derived is float64 from
    the integer counts.  ``a + b`` merges two runs with equal labels and k (exact: integers).  Holds
    host arrays only, so it pickles and loads where no GPU is visible."""

    _table = property(lambda self: self.counts)
    _norm = property(lambda self: self.S)

    def __init__(self, labels, counts, S, k):
        self.labels = list(labels)
        self.counts = np.ascontiguousarray(counts, np.int64)
        self.S, self.k = int(S), int(k)
        assert self.counts.shape == (len(self.labels), self.k + 1)

    def __add__(self, other):
        if not isinstance(other, CompositionHistogram):
            return NotImplemented
        if other.labels != self.labels or other.k != self.k:
            raise ValueError("composition histograms over different groups or panel sizes")
        return CompositionHistogram(self.labels, self.counts + other.counts, self.S + other.S, self.k)


def _is_device_tensor(a):
    return hasattr(a, "is_cuda") and a.is_cuda


def group_hist_device(d_panels, S, W, d_masks, G, bins, d_hist, d_status, stream):
    """Enqueue csa_group_hist_async on ``stream`` (a torch stream); nothing waits."""
    N.check(N.lib().csa_group_hist_async(N.ptr(d_panels), int(S), int(W), N.ptr(d_masks), int(G), int(bins),
                                         N.ptr(d_hist), N.ptr(d_status), ctypes.c_void_p(stream.cuda_stream)))


@contextlib.contextmanager
def _composition_input(panels, W, stream):
    """The two composition calls' preamble.  Yields (panels, their number, stream).  Host panels where no HIP
    device is visible come back as uint64[S, W] with stream None: the caller takes its numpy path.  Otherwise host
    rows are uploaded, a tensor that is no whole number of W-word rows is refused, and the block runs on the panels'
    device with ``stream`` (default: its current stream) current: it enqueues there and makes the one host copy."""
    on_device = _is_device_tensor(panels)
    if not on_device:
        panels = np.ascontiguousarray(panels, np.uint64).reshape(-1, W)
        try:
            import torch
            have = torch.cuda.is_available()
        except ImportError:
            have = False
        if not have:
            yield panels, len(panels), None
            return
    import torch
    dev = panels.device if on_device else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        st = stream or torch.cuda.current_stream(dev)
        with torch.cuda.stream(st):
            if not on_device:
                panels = torch.from_numpy(panels.view(np.int64).reshape(-1)).to(dev)
            if panels.numel() % W:
                raise ValueError("panels: %d words are no whole number of W = %d" % (panels.numel(), W))
            yield panels, panels.numel() // W, st


def group_composition(groups, panels, k, stream=None):
    """Composition of ``panels`` (packed host uint64[S, W], or the device tensor a run kept: int64 /
    uint64 words, S*W of them) over ``groups``: a CompositionHistogram with k + 1 bins per group.  With
    a HIP device the table comes from csa_group_hist_async (on ``stream``, default the panels' current
    stream; one host copy of the table and the status); without one, from ``group_hist_host``.  A
    panel holding more than k members of a group raises CsaError(CSA_E_INVALID) on either path."""
    k, G, W = int(k), len(groups), groups.W
    bins = k + 1
    with _composition_input(panels, W, stream) as (panels, S, st):
        if st is None:
            return CompositionHistogram(groups.labels, group_hist_host(groups.masks, panels, bins), S, k)
        import torch
        from .device import StatusBlock
        out = StatusBlock([("table", max(G * bins, 1))], torch.int64, panels.device, zero=True)
        group_hist_device(panels, S, W, groups.device_masks(panels.device), G, bins, out.views["table"], out.status, st)
        h, words = out.host()                      # the call's one host wait
    N.raise_status(words)
    return CompositionHistogram(groups.labels, h["table"][:G * bins].reshape(G, bins).copy(), S, k)


# ---- weighted composition: the same question for a LEXIMIN / XMIN portfolio ------------------------
#
# A portfolio's panels carry float64 probabilities, so hist[g][c] is a float64 sum, and float64 addition
# does not associate.  csa_group_whist_async fixes the order (ascending panel index, one add each);
# ``group_whist_host`` is that contract on the host and the yardstick the kernels are held to, bit for bit.

def _group_counts(masks, panels):
    """int64[P, G]: popcount(panel_p & mask_g), as ``group_hist_host`` counts (0/1 products, exact)."""
    G, W = masks.shape
    P = panels.shape[0]
    assert 64 * W < 1 << 24
    m = np.unpackbits(masks.view(np.uint8).reshape(G, -1), axis=1, bitorder="little").astype(np.float32)
    out = np.empty((P, G), np.int64)
    step = max(1, (1 << 24) // (64 * W))
    for off in range(0, P, step):
        x = np.unpackbits(panels[off:off + step].view(np.uint8).reshape(-1, 8 * W), axis=1, bitorder="little")
        out[off:off + step] = (x.astype(np.float32) @ m.T).astype(np.int64)
    return out


def group_whist_host(masks, panels, weights, bins, out=None):
    """csa_group_whist_async's contract on the host: float64[G, bins], hist[g][c] = the sum of weights[p]
    over the panels with popcount(panel_p & mask_g) == c, from +0.0 (or, with ``out=``, onto the values
    ``out`` holds: it is updated in place and returned), added in ASCENDING p, one float64 add each --
    a loop over the panels, each scattering its weight to one entry per group.  A count >= bins
    raises CsaError(CSA_E_INVALID) before anything is added, as the device's status block reports it."""
    masks = np.ascontiguousarray(masks, np.uint64)
    panels = np.ascontiguousarray(panels, np.uint64)
    weights = np.ascontiguousarray(weights, np.float64).reshape(-1)
    G, W = masks.shape
    P = panels.shape[0]
    assert panels.ndim == 2 and (P == 0 or panels.shape[1] == W) and len(weights) == P
    bins = int(bins)
    if out is None:
        out = np.zeros((G, bins), np.float64)
    assert out.shape == (G, bins) and out.dtype == np.float64 and out.flags.c_contiguous
    if G == 0 or P == 0:
        return out
    c = _group_counts(masks, panels)
    bad = np.argwhere(c >= bins)
    if len(bad):
        raise N.CsaError(N.CSA_E_INVALID, "group whist: panel %d holds %d members of group %d, bins = %d"
                         % (bad[0][0], c[bad[0][0], bad[0][1]], bad[0][1], bins))
    where = c + np.arange(G, dtype=np.int64) * bins            # [P, G]: one entry per group, all distinct
    flat = out.reshape(-1)
    for p in range(P):
        flat[where[p]] += weights[p]
    return out


class WeightedCompositionHistogram(_Composition):
    """``values[g][c]`` = summed weight of the portfolio's panels holding exactly c members of group g
    (host float64[G, k+1], the raw table, each entry added in portfolio order), over ``P`` panels of
    size ``k``; ``total`` is the portfolio-order sum of the weights from ``0.``.  The derived
    quantities describe the distribution ``values / total`` and mean what CompositionHistogram's do.
    Holds host arrays only, so it pickles and loads where no GPU is visible."""

    _table = property(lambda self: self.values)
    _norm = property(lambda self: self.total)

    def __init__(self, labels, values, total, P, k):
        self.labels = list(labels)
        self.values = np.ascontiguousarray(values, np.float64)
        self.total, self.P, self.k = float(total), int(P), int(k)
        assert self.values.shape == (len(self.labels), self.k + 1)


def portfolio_total(weights):
    """The portfolio-order sum of the weights from ``0.``, one float64 add each."""
    total = 0.
    for w in np.asarray(weights, np.float64).reshape(-1).tolist():
        total += w
    return total


def group_whist_device(d_panels, P, W, d_weights, d_masks, G, bins, d_hist, d_status, stream, accumulate=False):
    """Enqueue csa_group_whist_async on ``stream`` (a torch stream); nothing waits.  The count scratch is a
    tensor allocated here on that stream and lent to the call; it goes back to torch's allocator, which
    reuses it only for work ordered after this on the same stream."""
    import torch
    L = N.lib()
    need = int(L.csa_group_whist_scratch_bytes(int(P), int(G)))
    with torch.cuda.stream(stream):
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=d_hist.device)
    N.check(L.csa_group_whist_scratch(N.ptr(scratch), need))
    try:
        N.check(L.csa_group_whist_async(N.ptr(d_panels), int(P), int(W), N.ptr(d_weights), N.ptr(d_masks), int(G),
                                        int(bins), N.ptr(d_hist), N.CSA_GROUP_WHIST_ACCUMULATE if accumulate else 0,
                                        N.ptr(d_status), ctypes.c_void_p(stream.cuda_stream)))
    finally:
        N.check(L.csa_group_whist_scratch(None, 0))


def portfolio_group_composition(groups, panels, weights, k, stream=None):
    """Weighted composition of a portfolio over ``groups``: ``panels`` are its packed rows (host
    uint64[P, W], or a device tensor of P*W int64 / uint64 words), ``weights`` its P probabilities in
    portfolio order.  Returns a WeightedCompositionHistogram with k + 1 bins per group.  With a HIP
    device the table comes from csa_group_whist_async (on ``stream``, default the panels' current
    stream; one host copy of the table and the status); without one, from ``group_whist_host`` -- the
    same bits either way.  A panel holding more than k members of a group raises
    CsaError(CSA_E_INVALID) on either path."""
    k, G, W = int(k), len(groups), groups.W
    bins = k + 1
    weights = np.ascontiguousarray(weights, np.float64).reshape(-1)
    total = portfolio_total(weights)
    with _composition_input(panels, W, stream) as (panels, P, st):
        if P != len(weights):
            raise ValueError("%d panels with %d weights" % (P, len(weights)))
        if st is None:
            return WeightedCompositionHistogram(groups.labels, group_whist_host(groups.masks, panels, weights, bins),
                                                total, P, k)
        import torch
        from .device import StatusBlock
        d_masks = groups.device_masks(panels.device)
        d_w = torch.from_numpy(weights).to(panels.device)
        out = StatusBlock([("table", max(G * bins, 1))], torch.float64, panels.device)
        group_whist_device(panels, P, W, d_w, d_masks, G, bins, out.views["table"], out.status, st)
        h, words = out.host()                      # the call's one host wait
    N.raise_status(words)
    return WeightedCompositionHistogram(groups.labels, h["table"][:G * bins].reshape(G, bins).copy(), total, P, k)


# ---- panel multiplicities: the run as a distribution over whole panels -----------------------------
#
# LEXIMIN's portfolio is a distribution over panels; a LEGACY run of S draws is a sample of one.  The
# distinct count alone (found_panels) is a sample-size-limited number; how often each distinct panel was
# drawn gives the multiplicity spectrum, the sample coverage, a lower bound on the panels possible and
# the most likely panels.  On the device the list comes from csa_unique_mult_async (the dedupe's own
# table slots, csrc/multiplicity.inc); ``panel_multiplicities_host`` is the same contract in numpy.

def panel_multiplicities_host(panels):
    """(first int64[u], mult int64[u]) of packed panels uint64[S, W], ascending in ``first``: per distinct
    row the lowest index at which it occurs and the number of rows equal to it."""
    p = np.ascontiguousarray(panels, np.uint64)
    if p.ndim != 2:
        raise ValueError("panels must be uint64[S, W]")
    if len(p) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, mult = np.unique(p, axis=0, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    return first[order].astype(np.int64), mult[order].astype(np.int64)


def _pack_ids(panel, agent_ids, W):
    """One agent-id tuple -> uint64[W] row in encoding order; KeyError for an id that is no agent."""
    pos = {aid: q for q, aid in enumerate(agent_ids)}
    row = np.zeros(max(W, 1), np.uint64)
    for aid in panel:
        q = pos[aid]
        row[q >> 6] |= np.uint64(1) << np.uint64(q & 63)
    return row


class PanelDistribution:
    """How often each distinct panel of a run of ``S`` draws occurred.

    ``distinct`` = number of distinct panels D, ``spectrum`` (host int64, length ``max_multiplicity``
    + 1) with ``spectrum[j]`` = f_j, the panels seen exactly j times (``spectrum[0]`` is 0),
    ``sum_squares`` = the sum of the squared multiplicities.

    ``first`` / ``mult`` list, per distinct panel, its lowest draw index and its count, in any order:
    host arrays, or device tensors (as csa_unique_mult_async leaves them), which stay on the device
    until read.  ``panels``: the run's S packed panels (host uint64[S, W], or the device tensor of S*W
    words) from which ``top`` / ``count`` read the rows at the first indices; None when the panels
    were not kept -- then the spectrum and the estimators work and ``top`` / ``count`` raise
    RuntimeError.  Pickles hold host arrays only (the list, and the D distinct rows when panels were
    kept), so they load where no GPU is visible.

    Degenerate runs: S = 0 has no panels, spectrum [0], and coverage, chao1, collision_probability and
    max_probability all 0.0.  S = 1 has coverage 0.0, chao1 1.0 and collision_probability 0.0 (no pair
    of draws exists).  With f_1 = 0 (every panel seen at least twice) coverage is 1.0 and chao1 is D.
    """

    _where = "panels were not kept; only len() is available"  # analysis.PanelSet's message

    def __init__(self, S, first, mult, panels=None, n=0, agent_ids=None, spectrum=None, sum_squares=None):
        self.S = int(S)
        self._n, self._ids = int(n), agent_ids
        self._W = max((self._n + 63) // 64, 1)
        self._first, self._mult = first, mult      # any order; sorted by first index when first read
        self._sorted = False
        self._panels = panels                      # all S rows (indexed by first), or with _rows: the D rows
        self._rows = False
        self.distinct = int(len(first))
        if spectrum is None or sum_squares is None:
            m = self._host(mult)
            spectrum = np.bincount(m, minlength=1) if len(m) else np.zeros(1, np.int64)
            sum_squares = sum(int(x) * int(x) for x in m.tolist())
        self.spectrum = np.ascontiguousarray(spectrum, np.int64)
        self.sum_squares = int(sum_squares)
        self.max_multiplicity = len(self.spectrum) - 1
        j = np.arange(len(self.spectrum), dtype=np.int64)
        if int(self.spectrum.sum()) != self.distinct or int((self.spectrum * j).sum()) != self.S:
            raise ValueError("multiplicities of %d panels summing to %d do not describe %d draws of %d distinct panels"
                             % (int(self.spectrum.sum()), int((self.spectrum * j).sum()), self.S, self.distinct))

    @staticmethod
    def _host(a):
        if _is_device_tensor(a):
            return a.cpu().numpy().astype(np.int64) & 0xFFFFFFFF     # the device lists are uint32 words
        return np.asarray(a, np.int64)

    def __len__(self):
        return self.distinct

    def _f(self, j):
        return int(self.spectrum[j]) if j < len(self.spectrum) else 0

    def coverage(self):
        """Good-Turing sample coverage 1 - f_1 / S: the probability mass of the panels seen."""
        return 1 - self._f(1) / self.S if self.S else 0.0

    def chao1(self):
        """Chao1 lower bound on the number of possible panels, D + f_1 (f_1 - 1) / (2 (f_2 + 1))."""
        f1, f2 = self._f(1), self._f(2)
        return self.distinct + f1 * (f1 - 1) / (2 * (f2 + 1))

    def collision_probability(self):
        """The unbiased estimate of the sum of squared panel probabilities (LEXIMIN's concentration
        measure): (sum m^2 - S) / (S (S - 1)), the share of pairs of draws that gave the same panel."""
        S = self.S
        return (self.sum_squares - S) / (S * (S - 1)) if S > 1 else 0.0

    def max_probability(self):
        """The most frequent panel's share of the draws."""
        return self.max_multiplicity / self.S if self.S else 0.0

    def _sort(self):
        """The list ascending in first index (on the device while it is there)."""
        if not self._sorted:
            if _is_device_tensor(self._first):
                import torch
                f = self._first.to(torch.int64) & 0xFFFFFFFF
                f, order = torch.sort(f)
                self._first, self._mult = f, (self._mult.to(torch.int64) & 0xFFFFFFFF)[order]
            else:
                f, m = np.asarray(self._first, np.int64), np.asarray(self._mult, np.int64)
                order = np.argsort(f, kind="stable")
                self._first, self._mult = f[order], m[order]
                if self._rows:
                    self._panels = self._panels[order]
            self._sorted = True
        return self._first, self._mult

    def multiplicities(self):
        """Host ``(first int64[D], mult int64[D])`` ascending in first index."""
        f, m = self._sort()
        if _is_device_tensor(f):
            f, m = f.cpu().numpy(), m.cpu().numpy()
        return f.copy(), m.copy()

    def _panel_rows(self, where):
        """uint64[len(where), W]: the panels of the sorted list's entries ``where``."""
        if self._panels is None:
            raise RuntimeError(self._where)
        f, _ = self._sort()
        W = self._W
        if self._rows:
            return self._panels[np.asarray(where, np.int64)]
        if _is_device_tensor(self._panels):
            import torch
            at = f[torch.as_tensor(where, dtype=torch.int64, device=f.device)] if _is_device_tensor(f) else \
                torch.as_tensor(np.asarray(f)[np.asarray(where, np.int64)], device=self._panels.device)
            rows = self._panels[:self.S * W].view(self.S, W)[at.to(self._panels.device)]
            return np.ascontiguousarray(rows.cpu().numpy()).view(np.uint64).reshape(-1, W)
        fh = f.cpu().numpy() if _is_device_tensor(f) else f
        p = np.ascontiguousarray(self._panels).view(np.uint64).reshape(-1, W)
        return p[fh[np.asarray(where, np.int64)]]

    def _decode(self, row):
        from .instance import unpack_panel
        return tuple(self._ids[q] for q in unpack_panel(row, self._n))

    def top(self, m):
        """The ``m`` most frequent panels as ``[(sorted agent-id tuple, count), ...]``, most frequent
        first, ties in the order of their first draw.  A device list is sorted on the device and only
        the m rows are copied."""
        if self._panels is None:
            raise RuntimeError(self._where)
        f, mult = self._sort()
        m = max(0, min(int(m), self.distinct))
        if _is_device_tensor(mult):
            import torch
            cnt, where = torch.sort(mult, descending=True, stable=True)   # stable: first index breaks ties
            cnt, where = cnt[:m].cpu().numpy(), where[:m].cpu().numpy()
        else:
            where = np.argsort(-mult, kind="stable")[:m]
            cnt = mult[where]
        rows = self._panel_rows(where)
        return [(self._decode(r), int(c)) for r, c in zip(rows, cnt)]

    def count(self, panel):
        """How often ``panel`` (agent ids, any order) was drawn; 0 for a panel never drawn."""
        if self._panels is None:
            raise RuntimeError(self._where)
        row = _pack_ids(panel, self._ids, self._W)
        if self._table is not None and _is_device_tensor(self._table.rows):
            return int(_table_counts(self._table, row.reshape(1, -1))[0])     # log D row compares, one word copied
        f, mult = self._sort()
        if _is_device_tensor(self._panels) and not self._rows:
            import torch
            dev = self._panels.device
            at = f if _is_device_tensor(f) else torch.as_tensor(f, device=dev)
            rows = self._panels[:self.S * self._W].view(self.S, self._W)[at]
            hit = (rows == torch.from_numpy(row.view(np.int64)).to(dev)).all(dim=1).nonzero().reshape(-1).cpu().numpy()
        else:
            hit = np.flatnonzero((self._panel_rows(np.arange(self.distinct)) == row).all(axis=1))
        if len(hit) == 0:
            return 0
        return int(mult[int(hit[0])].item()) if _is_device_tensor(mult) else int(mult[hit[0]])

    _table = None

    def table(self):
        """The run as a sorted table: a RowTable of the D distinct panels ascending (``PanelSet.rows()``'s
        order) with ``first`` and ``mult``, what ``compare_panel_distributions`` and ``portfolio_overlap``
        join and search.  Kept panels on a device are sorted there (csa_rows_sort_unique_async; one host
        wait, for the length and the sum) and the table stays on that device; otherwise it is built on the
        host from the kept or pickled rows.  Its length must equal ``distinct`` and its multiplicities must
        sum to ``S``: RuntimeError otherwise.  Built once."""
        if self._table is not None:
            return self._table
        if self._panels is None:
            raise RuntimeError(self._where)
        W = self._W
        if _is_device_tensor(self._panels) and not self._rows and not rows_host_path():
            import torch
            dev = self._panels.device
            with torch.cuda.device(dev):
                t = rows_sort_unique_device(self._panels, self.S, W, torch.cuda.current_stream(dev), lists=True)
                d = min(int(t.length.item()), t.cap)
                s = int((t.mult[:d].to(torch.int64) & 0xFFFFFFFF).sum().item())
                if d != t.cap:       # a view would keep the sort's S-row output alive
                    t = RowTable(t.rows[:d].clone(), t.first[:d].clone(), t.mult[:d].clone(), t.length, d, W)
        else:
            f, m = self.multiplicities()
            rows = np.ascontiguousarray(self._panel_rows(np.arange(self.distinct)), np.uint64).reshape(-1, W)
            if len(rows):
                rows, at = np.unique(rows, axis=0, return_index=True)
                f, m = f[at], m[at]
            d, s = len(rows), int(m.sum())
            t = RowTable(rows, f, m, np.array([d], np.uint64), d, W)
        if d != self.distinct or s != self.S:
            raise RuntimeError("panel table: %d sorted rows whose multiplicities sum to %d, the run counted %d distinct "
                               "panels in %d draws" % (d, s, self.distinct, self.S))
        self._table = t
        return t

    def price(self, weights, scores=False):
        """The distinct panel with the largest weight sum, as a ``PanelPrice``: heuristic pricing of column
        generation over the panels this run drew.  ``weights``: a mapping agent id -> float covering every agent
        (KeyError otherwise) or a sequence in the instance's agent order; a weight that is not finite raises
        ValueError before anything is enqueued.  A table on a device is priced there (csa_rows_price_async:
        float64 sums in ascending agent order, ties to the lowest row of the sorted table; one host wait, for the
        best row's words), a host table through ``rows_price_host``.  ``scores=True`` returns ``(price,
        scores)``, the per-row scores left on the table's device as a float64 tensor (a numpy array for a host
        table)."""
        w = weight_vector(weights, self._ids)
        if not self.distinct:
            out = PanelPrice(frozenset(), float("-inf"), None, None, 0)
            return (out, np.zeros(0, np.float64)) if scores else out
        t = self.table()
        ops, device = _table_ops(t)
        best, sc = ops.price(t, self._n, w, scores=scores)
        if device:
            import torch
            with torch.cuda.stream(ops.stream):
                at = (best[:1] & 0xFFFFFFFF).clamp(0, t.cap - 1)
                lists = torch.stack([t.first, t.mult]).to(torch.int64)[:, at].reshape(-1) & 0xFFFFFFFF
                h = torch.cat([best, lists, t.rows.view(t.cap, t.W)[at].reshape(-1)]).cpu().numpy()
            sc = None if sc is None else sc[:self.distinct]
        else:
            at = min(int(best[0]), t.cap - 1)
            h = np.concatenate([best.view(np.int64), [int(t.first[at]), int(t.mult[at])],
                                np.asarray(t.rows).view(np.int64).reshape(-1, t.W)[at]])
        out = PanelPrice(frozenset(self._decode(h[4:].view(np.uint64))), float(h[1:2].view(np.float64)[0]), int(h[0]),
                         int(h[2]), int(h[3]))
        return (out, sc) if scores else out

    def initial_committees(self, rounds=None):
        """The reference's _generate_initial_committees (xmin.py:229-290, leximin.py:236-300) over the panels this
        run drew instead of an ILP over all feasible ones: ``rounds`` (default 3 n, leximin.py:373)
        multiplicative-weights rounds over the table -- on its device, csa_rows_mw_cover_async, two launches a
        round and no wait between them --, then every agent no pick covers gets the lowest row holding it
        (csa_rows_first_holder_async).  Returns ``(committees, covered_agents, output_lines)``, what
        _expand_distribution_leximin takes as ``initial_committees`` / ``initial_covered_agents``; the lines say
        which agents no drawn panel contains.  One host wait."""
        n = self._n
        rounds = 3 * n if rounds is None else int(rounds)
        if rounds < 0:
            raise ValueError("rounds must not be negative")
        if not self.distinct:
            none = np.full(n, NO_ROW, np.int64)
            return committees_from_cover(none[:0], none, none[:0], none, n, list(self._ids))
        t = self.table()
        ops, device = _table_ops(t)
        if device:
            import torch
            with torch.cuda.stream(ops.stream):
                w = torch.ones(n, dtype=torch.float64, device=ops.device)
                chosen = torch.zeros(t.cap, dtype=torch.uint8, device=ops.device)
                picks, _ = ops.mw_cover(t, n, rounds, w, chosen)
                first = ops.first_holder(t, n)
                h = torch.cat([picks.to(torch.int64) & 0xFFFFFFFF, first.to(torch.int64) & 0xFFFFFFFF,
                               _rows_at(t, picks, True).reshape(-1), _rows_at(t, first, True).reshape(-1)]).cpu().numpy()
            picks, first = h[:rounds], h[rounds:rounds + n]
            picked = h[rounds + n:rounds + n + rounds * t.W].reshape(rounds, t.W)
            holders = h[rounds + n + rounds * t.W:].reshape(n, t.W)
        else:
            picks, _ = ops.mw_cover(t, n, rounds, np.ones(n, np.float64), np.zeros(t.cap, np.uint8))
            first = ops.first_holder(t, n)
            picked, holders = _rows_at(t, picks, False), _rows_at(t, first, False)
        return committees_from_cover(picks, first, picked, holders, n, list(self._ids))

    def maximin(self, rounds=None, shrink=0.8, resync=16):
        """How fair could a lottery over exactly the panels this run drew be made?  The reference's
        _dual_leximin_stage with no fixed probabilities and P ranging over the drawn panels (xmin.py:293-321) --
        maximise the least selection probability of the agents some drawn panel holds -- solved as a zero-sum
        game by ``rounds`` (default 3 n, as ``initial_committees``) multiplicative-weights rounds over the
        sorted table: on its device csa_rows_maximin_async (plain launches, scores updated incrementally over
        each row's intersection with the pick and summed afresh every ``resync`` rounds, one host wait at the
        end), on the host ``rows_maximin_host``.  Returns a ``PanelMaximin``: the lottery of the picks as a
        portfolio, each agent's exact selection probability under it, and ``lower <= optimum <= upper``.  No LP
        solver is involved.  An empty run gives an empty result without a call; ValueError for rounds < 0,
        ``shrink`` outside [0.5, 1) or ``resync`` outside [1, 64]."""
        n = self._n
        rounds = 3 * n if rounds is None else int(rounds)
        n, rounds, shrink, resync = _maximin_arguments(n, self._W, rounds, shrink, resync)
        ids = list(self._ids)
        if not self.distinct:
            none = np.zeros(n, np.int64)
            return PanelMaximin(none[:0], none[:0].reshape(0, self._W), none, none, np.inf, n, ids)
        t = self.table()
        ops, device = _table_ops(t)
        if device:
            import torch
            with torch.cuda.stream(ops.stream):
                picks, b = ops.maximin(t, n, rounds, shrink, resync)
                h = torch.cat([b.block, b.weights.view(torch.int64), b.cover.to(torch.int64) & 0xFFFFFFFF,
                               picks.to(torch.int64) & 0xFFFFFFFF, _rows_at(t, picks, True).reshape(-1)]).cpu().numpy()
            upper = float(h[0:1].view(np.float64)[0])
            covered, cover = h[4:4 + n].view(np.float64) != 0.0, h[4 + n:4 + 2 * n]
            picks, picked = h[4 + 2 * n:4 + 2 * n + rounds], h[4 + 2 * n + rounds:].reshape(rounds, t.W)
        else:
            picks, st = ops.maximin(t, n, rounds, shrink, resync)
            upper, covered, cover = st.upper, st.weights != 0.0, st.cover
            picked = _rows_at(t, picks, False)
        return PanelMaximin(picks, picked, cover, covered, upper, n, ids)

    def nash(self, rounds=200, start="legacy"):
        """Which lottery over exactly the panels this run drew has the greatest geometric mean of selection
        probabilities (the third headline statistic of ``compute_prob_allocation_stats``), and how much of it
        does LEGACY leave on the table?  The Nash-welfare lottery -- the maximum product of the probabilities of
        the agents some drawn panel holds -- by ``rounds`` rounds of Cover's multiplicative iteration over the
        sorted table: on its device csa_rows_nash_async (plain launches; a START-only call, a clone of its
        marginals, the rounds, then one concatenated copy and one host wait), on the host ``rows_nash_host``.
        ``start="legacy"`` starts from the run's multiplicities / S, so round 0 is LEGACY's own lottery over these
        panels; ``start="uniform"`` from equal probabilities.  Returns a ``PanelNash``: the lottery, each agent's
        selection probability under it, and ``geometric_mean <= optimum <= upper``.  No LP solver is involved.
        An empty run gives an empty result without a call; ValueError for rounds < 0 or another ``start``."""
        n, rounds = self._n, int(rounds)
        if rounds < 0:
            raise ValueError("rounds must not be negative")
        if start not in ("legacy", "uniform"):
            raise ValueError("start must be 'legacy' or 'uniform', not %r" % (start,))
        ids = list(self._ids)
        if not self.distinct:
            return PanelNash(None, np.zeros(0), np.zeros(n), 0.0, np.zeros(n), 0.0, np.inf, 0, PRICE_NONE, n, ids)
        t = self.table()
        ops, device = _table_ops(t)
        mult = t.mult if start == "legacy" else None
        if device:
            import torch
            D = self.distinct
            with torch.cuda.stream(ops.stream):
                b = ops.nash(t, n, 0, mult, self.S)
                pi0, block0 = b.marginals.clone(), b.block.clone()
                b = ops.nash(t, n, rounds, state=b)
                h = torch.cat([b.block, block0[3:4], b.marginals.view(torch.int64), pi0.view(torch.int64),
                               b.prob[:D].view(torch.int64)]).cpu().numpy()
            f = lambda a: a.view(np.float64)
            st = NashState(f(h[5 + 2 * n:]), None, f(h[5:5 + n]), float(f(h[0:1])[0]), int(h[1]), int(h[2]),
                           float(f(h[3:4])[0]))
            pi0, psum0 = f(h[5 + n:5 + 2 * n]), float(f(h[4:5])[0])
        else:
            st0 = ops.nash(t, n, 0, mult, self.S)
            st = ops.nash(t, n, rounds, state=st0)
            pi0, psum0 = st0.marginals, st0.psum
        return PanelNash(t, st.prob, st.marginals, st.psum, pi0, psum0, st.ratio, st.rounds, st.best_row, n, ids)

    def __getstate__(self):
        f, m = self.multiplicities()
        rows = self._panel_rows(np.arange(self.distinct)) if self._panels is not None else None
        return {"S": self.S, "n": self._n, "ids": self._ids, "first": f, "mult": m, "rows": rows,
                "spectrum": self.spectrum, "sum_squares": self.sum_squares}

    def __setstate__(self, st):
        self.S, self._n, self._ids = st["S"], st["n"], st["ids"]
        self._W = max((self._n + 63) // 64, 1)
        self._first, self._mult, self._sorted = st["first"], st["mult"], True
        self._panels, self._rows = st["rows"], st["rows"] is not None
        self.distinct = len(self._first)
        self.spectrum, self.sum_squares = st["spectrum"], st["sum_squares"]
        self.max_multiplicity = len(self.spectrum) - 1


def _plain_distribution(state):
    """Unpickling of a ShardedPanelDistribution: the host-list PanelDistribution it was materialised to."""
    d = PanelDistribution.__new__(PanelDistribution)
    d.__setstate__(state)
    return d


class ShardedPanelDistribution(PanelDistribution):
    """The PanelDistribution of a sharded run (distributed.legacy_panel_distribution_distributed): ``S``,
    ``distinct``, ``spectrum``, ``sum_squares``, ``max_multiplicity`` and the estimators are the WHOLE job's,
    on every rank (the owners' records summed in the call's all_reduce), under the constructor's consistency
    check.  What a rank holds of the list itself:

    ``owned()``: this rank's owner list, host ``(first, mult)`` ascending in first -- the panels whose
    h1 % world is this rank, with the job's lowest draw index and the job's count of each.

    ``candidates``: ``(first, mult)`` of every owner's ``top_keep`` most frequent entries (any order).
    Multiplicity descending, then first index ascending, is a total order, so the job's ``top_keep``
    most frequent panels are among them: ``top(m)`` for m <= ``top_keep`` is answered from them, their rows
    re-drawn by index, one panel each, through ``redraw.draw(first, 1)`` -- no collective, any rank, alone.

    ``multiplicities()``, ``count()``, ``top(m > top_keep)`` and pickling need the whole list: they re-draw
    the job's panels [0, S) on this rank (``redraw()``, the distributed.PanelRedraw of the run's
    found_panels) and count them -- on the device where the re-draw streams (``PanelRedraw.table``: the sorted
    table of distinct rows with first index and count, D entries copied and ordered by first index here), on
    the host otherwise (``panel_multiplicities_host``); from then on the object is a host-list
    distribution, and pickles as a plain PanelDistribution.  A materialised list whose spectrum differs from
    the reduced one raises RuntimeError.  ``redraw=None`` (the panels were not kept): the estimators and
    ``owned()`` work, the others raise RuntimeError with PanelSet's message."""

    def __init__(self, S, distinct, spectrum, sum_squares, owned_first, owned_mult, candidates=None, top_keep=0,
                 redraw=None, n=0, agent_ids=None):
        self.S, self.distinct = int(S), int(distinct)
        self.spectrum = np.ascontiguousarray(spectrum, np.int64)
        self.sum_squares = int(sum_squares)
        self.max_multiplicity = len(self.spectrum) - 1
        j = np.arange(len(self.spectrum), dtype=np.int64)
        if int(self.spectrum.sum()) != self.distinct or int((self.spectrum * j).sum()) != self.S:
            raise ValueError("multiplicities of %d panels summing to %d do not describe %d draws of %d distinct panels"
                             % (int(self.spectrum.sum()), int((self.spectrum * j).sum()), self.S, self.distinct))
        self._owned = (owned_first, owned_mult)
        cf, cm = candidates if candidates is not None else ((), ())
        cf, cm = np.asarray(cf, np.int64).reshape(-1), np.asarray(cm, np.int64).reshape(-1)
        order = np.lexsort((cf, -cm))
        self.top_keep = max(0, int(top_keep))
        self._cand = (cf[order][:self.top_keep], cm[order][:self.top_keep])
        self._cand_rows = {}
        self._whole = False                         # the whole list is on this rank (materialised)
        self._first = self._mult = self._panels = None
        self._sorted, self._rows = False, False
        self.bind(redraw, n, agent_ids)

    def bind(self, redraw, n, agent_ids):
        """The run's PanelRedraw (None: panels not kept) and the encoding's agents, to decode rows with."""
        self._redraw = redraw
        self._n, self._ids = int(n), agent_ids
        self._W = max((self._n + 63) // 64, 1)
        return self

    def owned(self):
        """Host ``(first int64[u], mult int64[u])`` ascending in first: this rank's owner list."""
        f, m = (self._host(a) for a in self._owned)
        order = np.argsort(f, kind="stable")
        return f[order], m[order]

    def _materialise(self):
        if self._whole:
            return
        if self._redraw is None:
            raise RuntimeError(self._where)
        if getattr(self._redraw, "streams", None) is not None and self._redraw.streams():
            # the sorted table, folded on the device chunk by chunk: D entries reach the host, ordered by
            # first index here
            rows, first, mult = self._redraw.table(self.distinct, lists=True)
            order = np.argsort(first, kind="stable")
            first, mult, kept = first[order], mult[order], rows[order]
        else:
            panels = np.ascontiguousarray(self._redraw(), np.uint64).reshape(self.S, -1)
            first, mult = panel_multiplicities_host(panels)
            kept = panels[first]
        spectrum = np.bincount(mult, minlength=1) if len(mult) else np.zeros(1, np.int64)
        if len(first) != self.distinct or not np.array_equal(spectrum, self.spectrum):
            raise RuntimeError("panel multiplicities: the re-drawn panels hold %d distinct panels with another "
                               "spectrum than the run reduced over %d" % (len(first), self.distinct))
        self._first, self._mult, self._sorted = first, mult, True
        self._panels, self._rows = kept, True
        self._whole = True

    def multiplicities(self):
        self._materialise()
        return super().multiplicities()

    def count(self, panel):
        self._materialise()
        return super().count(panel)

    def table(self):
        self._materialise()
        return super().table()

    def top(self, m):
        m = max(0, min(int(m), self.distinct))
        if self._whole or m > len(self._cand[0]):
            self._materialise()
            return super().top(m)
        if self._redraw is None:
            raise RuntimeError(self._where)
        out = []
        for f, c in zip(self._cand[0][:m].tolist(), self._cand[1][:m].tolist()):
            if f not in self._cand_rows:
                row = np.ascontiguousarray(self._redraw.draw(f, 1), np.uint64).reshape(-1)
                self._cand_rows[f] = self._decode(row)
            out.append((self._cand_rows[f], c))
        return out

    def __reduce__(self):
        self._materialise()
        return _plain_distribution, (PanelDistribution.__getstate__(self),)


def unique_mult_device(d_hashes, d_panels, S, W, d_status, stream, n_bins=4096):
    """Enqueue csa_unique_mult_async + csa_mult_spectrum_async over a batch's device hashes and panels on
    ``stream`` (a torch stream); nothing waits.  Returns (first, mult, out): two int32 tensors of
    max(S, 1) uint32 words, and int64 ``out`` = [list length, spectrum[n_bins], overflow, max,
    sum m^2, sum m].  The scratch is allocated here on that stream and goes back to torch's allocator,
    which reuses it only for work ordered after this on the same stream."""
    import torch
    L = N.lib()
    S, W, n_bins = int(S), int(W), int(n_bins)
    dev = d_hashes.device
    with torch.cuda.stream(stream):
        need = int(L.csa_unique_mult_scratch_bytes(S))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        first = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
        mult = torch.empty(max(S, 1), dtype=torch.int32, device=dev)
        out = torch.empty(1 + n_bins + 4, dtype=torch.int64, device=dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    N.check(L.csa_unique_mult_async(N.ptr(d_hashes), N.ptr(d_panels), S, W, N.ptr(scratch), need, N.ptr(first),
                                    N.ptr(mult), N.ptr(out), N.ptr(d_status), sp))
    N.check(L.csa_mult_spectrum_async(N.ptr(mult), N.ptr(out), S, N.ptr(out[1:]), n_bins, N.ptr(out[1 + n_bins:]), sp))
    return first, mult, out


# --- the distinct panels as a sorted table (csrc/distinct_rows.inc) ---------------------------------------
# found_panels read on the device: the distinct rows in PanelSet.rows()'s order (np.unique(axis=0): word 0
# most significant, unsigned), each with its lowest draw index and its count.  csa_rows_sort_unique_async
# makes the table of one chunk, csa_rows_merge_unique_async folds it into the table so far, so neither the
# host nor the device ever holds a sharded job's S x W words.  The ``*_host`` functions are the two
# contracts in numpy (the checkers); HostRowTables / DeviceRowTables put either pair behind the one
# interface distributed.PanelRedraw.table streams through.

def rows_host_path():
    """CSA_ROWS_HOST=1: read found_panels through the host np.unique path everywhere (A/B runs)."""
    import os
    return os.environ.get("CSA_ROWS_HOST") == "1"


def rows_sort_unique_host(rows, index_base=0):
    """``(rows uint64[D, W], first int64[D], mult int64[D])`` of packed rows uint64[n, W]: the distinct rows
    ascending (word 0 most significant, unsigned), per row ``index_base`` + the lowest input index holding it
    and the number of inputs holding it -- csa_rows_sort_unique_async's contract."""
    p = np.ascontiguousarray(rows, np.uint64)
    if p.ndim != 2:
        raise ValueError("rows must be uint64[n, W]")
    if len(p) == 0:
        return p.copy(), np.zeros(0, np.int64), np.zeros(0, np.int64)
    u, first, mult = np.unique(p, axis=0, return_index=True, return_counts=True)
    return u, first.astype(np.int64) + int(index_base), mult.astype(np.int64)


def rows_merge_unique_host(a, b):
    """The sorted distinct union of two ``(rows, first, mult)`` tables, each sorted and distinct: a row in
    both gets the lower ``first`` and the summed ``mult`` -- csa_rows_merge_unique_async's contract."""
    ra, rb = (np.ascontiguousarray(t[0], np.uint64) for t in (a, b))
    if not len(ra) or not len(rb):
        r, f, m = b if not len(ra) else a
        return np.ascontiguousarray(r, np.uint64).copy(), np.asarray(f, np.int64).copy(), np.asarray(m, np.int64).copy()
    u, inv = np.unique(np.concatenate([ra, rb]), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    first = np.full(len(u), np.iinfo(np.int64).max, np.int64)
    mult = np.zeros(len(u), np.int64)
    np.minimum.at(first, inv, np.concatenate([np.asarray(a[1], np.int64), np.asarray(b[1], np.int64)]))
    np.add.at(mult, inv, np.concatenate([np.asarray(a[2], np.int64), np.asarray(b[2], np.int64)]))
    return u, first, mult


class RowTable:
    """A sorted distinct-row table of capacity ``cap`` rows: ``rows`` [cap, W], ``first`` / ``mult`` [cap]
    (uint32 words), ``length`` one uint64 word beside them (device tensors, or numpy arrays on the host)."""

    def __init__(self, rows, first, mult, length, cap, W):
        self.rows, self.first, self.mult, self.length, self.cap, self.W = rows, first, mult, length, int(cap), int(W)


def table_bytes(cap, chunk, W):
    """Device bytes of a streamed re-draw: the table of ``cap`` rows and its ping-pong twin, one chunk (its
    panels and its sorted table) and the larger of the two scratches."""
    L = N.lib()
    cap, chunk, W = max(int(cap), 1), max(int(chunk), 1), max(int(W), 1)
    one = lambda rows: rows * (8 * W + 8)
    return 2 * one(cap) + 8 * chunk * W + one(chunk) + \
        max(int(L.csa_rows_sort_scratch_bytes(chunk, W)), int(L.csa_rows_merge_scratch_bytes(cap, chunk, W)))


class HostRowTables:
    """The table operations on numpy arrays through the host mirrors: what DeviceRowTables does on a GPU, for
    draws that hand out host chunks behind the device interface (tests; the C oracle standing in for a GPU).
    ``free_bytes``: what the size guard is told is free."""

    def __init__(self, free_bytes=1 << 62):
        self._free = int(free_bytes)
        self.status = np.zeros(4, np.uint32)

    def free_bytes(self):
        return self._free

    def new_table(self, cap, W):
        cap, W = max(int(cap), 1), max(int(W), 1)
        return RowTable(np.zeros((cap, W), np.uint64), np.zeros(cap, np.int64), np.zeros(cap, np.int64),
                        np.zeros(1, np.uint64), cap, W)

    def sort_unique(self, rows, n, W, index_base):
        r, f, m = rows_sort_unique_host(np.asarray(rows).view(np.uint64).reshape(-1, max(W, 1))[:n], index_base)
        return RowTable(r, f, m, np.array([len(r)], np.uint64), max(n, 1), W)

    def merge(self, a, b, out):
        la, lb = (min(int(t.length[0]), t.cap) for t in (a, b))
        r, f, m = rows_merge_unique_host((a.rows[:la], a.first[:la], a.mult[:la]),
                                         (b.rows[:lb], b.first[:lb], b.mult[:lb]))
        if len(r) > out.cap and not self.status[0]:
            self.status[:] = (N.CSA_E_UNSUPPORTED, 0xFFFFFFFF, 0xFFFFFFFF, 0)
        keep = min(len(r), out.cap)
        out.rows[:keep], out.first[:keep], out.mult[:keep], out.length[0] = r[:keep], f[:keep], m[:keep], len(r)
        return out

    def join(self, a, b, select, scales=(1, 1), cap_out=None):
        """rows_join_host over two tables' first ``length`` rows, as a RowJoin of numpy arrays; more selected rows
        than the capacity, or a sum beyond 64 bits, sets CSA_E_UNSUPPORTED in ``status``."""
        la, lb = (min(int(t.length[0]), t.cap) for t in (a, b))
        side = lambda t, n: (t.rows[:n], None if t.mult is None else np.asarray(t.mult[:n], np.int64) & 0xFFFFFFFF)
        r, ma, mb, length, record = rows_join_host(side(a, la), side(b, lb), select, scales)
        cap = _join_cap(a, b, select) if cap_out is None else int(cap_out)
        if (length > cap or record[10]) and not self.status[0]:
            self.status[:] = (N.CSA_E_UNSUPPORTED, 0xFFFFFFFF, 0xFFFFFFFF, 0)
        return RowJoin(r[:cap], ma[:cap], mb[:cap], np.array([length], np.uint64), record, cap)

    def find(self, table, queries):
        return rows_find_host(table.rows[:min(int(table.length[0]), table.cap)], queries)

    def _valid(self, table):
        return np.asarray(table.rows).view(np.uint64).reshape(-1, table.W)[:min(int(table.length[0]), table.cap)]

    def price(self, table, n, weights, index_base=0, best=None, scores=False):
        """rows_price_host over the table's first ``length`` rows: ``(best uint64[2], scores or None)``, the
        best as csa_rows_price_async leaves it (index, score bits); ``best`` given: accumulated onto, in place."""
        w = np.asarray(weights, np.float64).reshape(-1)[:n]
        old = None if best is None else (int(best[0]), float(best[1:2].view(np.float64)[0]))
        at, value, sc = rows_price_host(self._valid(table), w, index_base, old)
        out = np.zeros(2, np.uint64) if best is None else best
        out[0], out[1:2].view(np.float64)[0] = at, value
        return out, (sc if scores else None)

    def mw_cover(self, table, n, rounds, weights, chosen, pick_scores=False):
        """rows_mw_cover_host; ``weights`` (float64[n]) and ``chosen`` (uint8[cap]) are updated in place.  Returns
        ``(picks int64[rounds], pick scores or None)``."""
        d = min(int(table.length[0]), table.cap)
        picks, w, ch, ps = rows_mw_cover_host(self._valid(table), weights[:n], chosen[:d], rounds)
        weights[:n], chosen[:d] = w, ch
        return picks, (ps if pick_scores else None)

    def first_holder(self, table, n):
        return rows_first_holder_host(self._valid(table), n)

    def maximin(self, table, n, rounds, shrink=0.8, resync=16, state=None):
        """rows_maximin_host over the table's first ``length`` rows: ``(picks int64[rounds], MaximinState)``."""
        return rows_maximin_host(self._valid(table), n, rounds, shrink, resync, state)

    def nash(self, table, n, rounds, mult=None, total=None, state=None):
        """rows_nash_host over the table's first ``length`` rows: a NashState.  ``mult`` = one count per row of
        the table (its first ``length`` are used) with their ``total``, or None for the uniform start."""
        d = min(int(table.length[0]), table.cap)
        return rows_nash_host(self._valid(table), n, rounds, None if mult is None else np.asarray(mult)[:d], total, state)

    def marginals(self, table, n, prob):
        """rows_marginals_host over the table's first ``length`` rows: ``(pi float64[n], psum)``."""
        return rows_marginals_host(self._valid(table), np.asarray(prob)[:min(int(table.length[0]), table.cap)], n)

    def read(self, table, lists, draw_status=None):
        d = min(int(table.length[0]), table.cap)
        words = np.concatenate([np.zeros(4, np.uint32) if draw_status is None else np.asarray(draw_status, np.uint32),
                                self.status])
        return (words, int(table.length[0]), table.rows[:d].copy(),
                table.first[:d].copy() if lists else None, table.mult[:d].copy() if lists else None)


def rows_sort_unique_device(d_rows, n_rows, W, stream, index_base=0, lists=True):
    """Enqueue csa_rows_sort_unique_async over ``n_rows`` device rows (int64 words, row-major) on ``stream`` (a
    torch stream); nothing waits.  Returns a RowTable of capacity max(n_rows, 1) on the rows' device (``first``
    / ``mult`` None without ``lists``).  The scratch comes from torch's allocator on that stream, which reuses
    it only for work ordered after this on the same stream."""
    import torch
    L = N.lib()
    n, W = int(n_rows), int(W)
    dev = d_rows.device
    cap = max(n, 1)
    with torch.cuda.stream(stream):
        need = int(L.csa_rows_sort_scratch_bytes(n, W))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        rows = torch.empty((cap, W), dtype=torch.int64, device=dev)
        first = torch.empty(cap, dtype=torch.int32, device=dev) if lists else None
        mult = torch.empty(cap, dtype=torch.int32, device=dev) if lists else None
        length = torch.empty(1, dtype=torch.int64, device=dev)
    N.check(L.csa_rows_sort_unique_async(N.ptr(d_rows), n, W, int(index_base), N.ptr(scratch), need, N.ptr(rows),
                                         N.ptr(first), N.ptr(mult), N.ptr(length), None,
                                         ctypes.c_void_p(stream.cuda_stream)))
    return RowTable(rows, first, mult, length, cap, W)


def rows_merge_unique_device(a, b, out, d_status, stream):
    """Enqueue csa_rows_merge_unique_async of RowTables ``a`` and ``b`` into ``out`` (all on one device, lengths
    read there) on ``stream``; nothing waits.  A union beyond ``out.cap`` raises CSA_E_UNSUPPORTED in
    ``d_status`` (int32[4] on the device).  Scratch as in rows_sort_unique_device.  Returns ``out``."""
    import torch
    L = N.lib()
    W = a.W
    with torch.cuda.stream(stream):
        need = int(L.csa_rows_merge_scratch_bytes(a.cap, b.cap, W))
        scratch = torch.empty(need, dtype=torch.uint8, device=out.rows.device)
    N.check(L.csa_rows_merge_unique_async(N.ptr(a.rows), N.ptr(a.first), N.ptr(a.mult), N.ptr(a.length), a.cap,
                                          N.ptr(b.rows), N.ptr(b.first), N.ptr(b.mult), N.ptr(b.length), b.cap, W,
                                          N.ptr(scratch), need, N.ptr(out.rows), N.ptr(out.first), N.ptr(out.mult),
                                          out.cap, N.ptr(out.length), N.ptr(d_status),
                                          ctypes.c_void_p(stream.cuda_stream)))
    return out


class DeviceRowTables:
    """The table operations on ``device``, enqueued on ``stream``: csa_rows_sort_unique_async and
    csa_rows_merge_unique_async, with one status block for every merge of a re-draw."""

    def __init__(self, device, stream):
        import torch
        self.device, self.stream = device, stream
        with torch.cuda.stream(stream):
            self.status = torch.zeros(4, dtype=torch.int32, device=device)

    def free_bytes(self):
        """The device's free memory (torch.cuda.mem_get_info).  Blocks torch's caching allocator holds but has
        not handed out are not in it, though the table's tensors could reuse them: right after a large call
        the guard errs on the side of refusing (torch.cuda.empty_cache() returns them to the figure)."""
        import torch
        return int(torch.cuda.mem_get_info(self.device)[0])

    def new_table(self, cap, W):
        import torch
        cap, W = max(int(cap), 1), max(int(W), 1)
        with torch.cuda.stream(self.stream):
            return RowTable(torch.empty((cap, W), dtype=torch.int64, device=self.device),
                            torch.empty(cap, dtype=torch.int32, device=self.device),
                            torch.empty(cap, dtype=torch.int32, device=self.device),
                            torch.zeros(1, dtype=torch.int64, device=self.device), cap, W)

    def sort_unique(self, rows, n, W, index_base):
        return rows_sort_unique_device(rows, n, W, self.stream, index_base)

    def merge(self, a, b, out):
        return rows_merge_unique_device(a, b, out, self.status, self.stream)

    def join(self, a, b, select, scales=(1, 1), cap_out=None, rows=True, mults=True):
        return rows_join_device(a, b, select, self.status, self.stream, scales, cap_out, rows, mults)

    def find(self, table, d_queries, n_queries):
        return rows_find_device(table, d_queries, n_queries, self.stream)

    def price(self, table, n, weights, index_base=0, best=None, scores=False):
        return rows_price_device(table, n, weights, self.stream, index_base, best, scores)

    def mw_cover(self, table, n, rounds, weights, chosen, pick_scores=False):
        return rows_mw_cover_device(table, n, rounds, weights, chosen, self.stream, pick_scores)

    def first_holder(self, table, n):
        return rows_first_holder_device(table, n, self.stream)

    def maximin(self, table, n, rounds, shrink=0.8, resync=16, state=None):
        """rows_maximin_device on this stream: ``(picks, MaximinBuffers)``, nothing waits."""
        return rows_maximin_device(table, n, rounds, shrink, resync, state, self.stream)

    def nash(self, table, n, rounds, mult=None, total=None, state=None):
        """rows_nash_device on this stream: a NashBuffers, nothing waits."""
        return rows_nash_device(table, n, rounds, mult, total, state, self.stream)

    def marginals(self, table, n, d_prob):
        """rows_marginals_device on this stream: ``(pi, psum)`` as float64 tensors, nothing waits."""
        return rows_marginals_device(table, n, d_prob, self.stream)

    def read(self, table, lists, draw_status=None):
        """The one host wait: [draw status | table status | length], then the D rows (and lists)."""
        import torch
        with torch.cuda.stream(self.stream):
            ds = draw_status if draw_status is not None else torch.zeros_like(self.status)
            head = torch.cat([ds.view(torch.int64), self.status.view(torch.int64), table.length]).cpu().numpy()
            words, length = head[:4].view(np.uint32).copy(), int(head[4])
            d = min(length, table.cap)
            rows = np.ascontiguousarray(table.rows[:d].cpu().numpy()).view(np.uint64).reshape(d, table.W)
            first = mult = None
            if lists:
                first = table.first[:d].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
                mult = table.mult[:d].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        return words, length, rows, first, mult


# --- two tables side by side (csrc/rows_join.inc) -----------------------------------------------------------
# The join of two sorted distinct-row tables and the lookup of a few rows in one: what the set algebra of
# analysis.PanelSet, the two-run comparison and the portfolio overlap are made of.  ``rows_join_host`` and
# ``rows_find_host`` are csa_rows_join_async's and csa_rows_find_async's contracts in numpy.

JOIN_ONLY_A, JOIN_ONLY_B, JOIN_BOTH = 1, 2, 4
JOIN_RECORD = ("union", "shared", "only_a", "only_b", "sum_a", "sum_b", "shared_a", "shared_b", "cross", "overlap",
               "overflow")
FIND_MISSING = 0xFFFFFFFF


class RowJoin:
    """What a join gives: the selected union rows ``rows`` [cap, W] ascending with ``mult_a`` / ``mult_b`` [cap]
    (0 where the row is absent from that side; any of the three None when not asked for), their number
    ``length`` (one word) and the 11-word ``record`` over the whole union (JOIN_RECORD).  Device tensors, or
    numpy arrays on the host, where ``record`` is a list of Python integers."""

    def __init__(self, rows, mult_a, mult_b, length, record, cap):
        self.rows, self.mult_a, self.mult_b, self.length, self.record, self.cap = rows, mult_a, mult_b, length, record, cap


def _join_side(t):
    rows = np.ascontiguousarray(t[0], np.uint64)
    if rows.ndim != 2:
        raise ValueError("rows must be uint64[n, W]")
    mult = np.ones(len(rows), np.int64) if t[1] is None else np.asarray(t[1], np.int64).reshape(-1)
    if len(mult) != len(rows):
        raise ValueError("one multiplicity per row")
    return rows, mult


def rows_join_host(a, b, select, scales=(1, 1)):
    """csa_rows_join_async's contract: ``a`` and ``b`` are ``(rows uint64[n, W], mult or None)``, each sorted and
    distinct (None: every multiplicity 1).  Returns ``(rows, mult_a, mult_b, length, record)``: the union rows
    whose class (1 only in a, 2 only in b, 4 in both) is in the mask ``select``, ascending, their multiplicities
    on either side (int64, 0 where absent), their number, and the record of the whole union as 11 Python
    integers (JOIN_RECORD; words 8 and 9 modulo 2^64 with word 10 = 1 when either did not fit)."""
    select, (sa, sb) = int(select), (int(s) for s in scales)
    if not 0 <= select <= 7 or not (0 <= sa < 1 << 32 and 0 <= sb < 1 << 32):
        raise ValueError("select is a mask of 1 | 2 | 4 and the scales are below 2^32")
    (ra, ma), (rb, mb) = _join_side(a), _join_side(b)
    W = ra.shape[1] if len(ra) or not len(rb) else rb.shape[1]
    if len(ra) + len(rb) == 0:
        return np.zeros((0, W), np.uint64), np.zeros(0, np.int64), np.zeros(0, np.int64), 0, [0] * 11
    u, inv = np.unique(np.concatenate([ra.reshape(-1, W), rb.reshape(-1, W)]), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    xa, xb = np.zeros(len(u), np.int64), np.zeros(len(u), np.int64)
    in_a, in_b = np.zeros(len(u), np.bool_), np.zeros(len(u), np.bool_)
    xa[inv[:len(ra)]], in_a[inv[:len(ra)]] = ma, True
    xb[inv[len(ra):]], in_b[inv[len(ra):]] = mb, True
    cls = np.where(in_a & in_b, JOIN_BOTH, np.where(in_a, JOIN_ONLY_A, JOIN_ONLY_B))
    both = cls == JOIN_BOTH
    pa, pb = xa[both].tolist(), xb[both].tolist()
    cross = sum(x * y for x, y in zip(pa, pb))
    overlap = sum(min(x * sb, y * sa) for x, y in zip(pa, pb))
    record = [len(u), int(both.sum()), int((cls == JOIN_ONLY_A).sum()), int((cls == JOIN_ONLY_B).sum()),
              sum(ma.tolist()), sum(mb.tolist()), sum(pa), sum(pb), cross & (2 ** 64 - 1), overlap & (2 ** 64 - 1),
              int(cross >= 2 ** 64 or overlap >= 2 ** 64)]
    keep = (cls & select) != 0
    return u[keep], xa[keep], xb[keep], int(keep.sum()), record


def rows_find_host(table_rows, queries):
    """csa_rows_find_async's contract: int64[Q], per query row the index of the equal row of the sorted distinct
    ``table_rows``, or FIND_MISSING.  The queries need be neither sorted nor distinct."""
    t = np.ascontiguousarray(table_rows, np.uint64)
    q = np.ascontiguousarray(queries, np.uint64)
    if t.ndim != 2 or q.ndim != 2 or (len(t) and len(q) and t.shape[1] != q.shape[1]):
        raise ValueError("table and queries must be uint64[n, W] of one W")
    out = np.full(len(q), FIND_MISSING, np.int64)
    if not len(t) or not len(q):
        return out
    u, inv = np.unique(np.concatenate([t, q]), axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    where = np.full(len(u), FIND_MISSING, np.int64)
    where[inv[:len(t)]] = np.arange(len(t))
    return where[inv[len(t):]]


def _join_cap(a, b, select):
    """The most rows a join of capacities ``a.cap`` and ``b.cap`` can select."""
    most = (a.cap if select & JOIN_ONLY_A else 0) + (b.cap if select & JOIN_ONLY_B else 0) + \
        (min(a.cap, b.cap) if select & JOIN_BOTH else 0)
    return min(most, a.cap + b.cap)


def rows_join_device(a, b, select, d_status, stream, scales=(1, 1), cap_out=None, rows=True, mults=True):
    """Enqueue csa_rows_join_async of RowTables ``a`` and ``b`` (on one device, lengths read there; a ``mult``
    of None counts every row once) on ``stream``; nothing waits.  Returns a RowJoin on that device: outputs of
    ``cap_out`` rows (default: the most ``select`` can give; ``rows`` / ``mults`` False: not written), the length
    and the record as int64 tensors.  More selected rows than ``cap_out``, or a sum beyond 64 bits, raises
    CSA_E_UNSUPPORTED in ``d_status`` (int32[4] on the device).  Scratch as in rows_sort_unique_device."""
    import torch
    L = N.lib()
    W, select = a.W, int(select)
    dev = a.length.device
    cap = _join_cap(a, b, select) if cap_out is None else int(cap_out)
    with torch.cuda.stream(stream):
        need = int(L.csa_rows_join_scratch_bytes(a.cap, b.cap, W))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((cap, W), dtype=torch.int64, device=dev) if rows and select else None
        mult_a = torch.empty(cap, dtype=torch.int32, device=dev) if mults and select else None
        mult_b = torch.empty(cap, dtype=torch.int32, device=dev) if mults and select else None
        length = torch.empty(1, dtype=torch.int64, device=dev)
        record = torch.empty(len(JOIN_RECORD), dtype=torch.int64, device=dev)
    N.check(L.csa_rows_join_async(N.ptr(a.rows), N.ptr(a.mult), N.ptr(a.length), a.cap,
                                  N.ptr(b.rows), N.ptr(b.mult), N.ptr(b.length), b.cap, W, select,
                                  int(scales[0]), int(scales[1]), N.ptr(scratch), need, N.ptr(out), N.ptr(mult_a),
                                  N.ptr(mult_b), cap, N.ptr(length), N.ptr(record), N.ptr(d_status),
                                  ctypes.c_void_p(stream.cuda_stream)))
    return RowJoin(out, mult_a, mult_b, length, record, cap)


def rows_find_device(table, d_queries, n_queries, stream):
    """Enqueue csa_rows_find_async of ``n_queries`` device rows (int64 words, row-major) in RowTable ``table`` on
    ``stream``; nothing waits.  Returns an int32 tensor of n_queries uint32 words: the index, or FIND_MISSING."""
    import torch
    n = int(n_queries)
    with torch.cuda.stream(stream):
        out = torch.empty(max(n, 1), dtype=torch.int32, device=table.length.device)
    N.check(N.lib().csa_rows_find_async(N.ptr(table.rows), N.ptr(table.length), table.cap, table.W, N.ptr(d_queries),
                                        n, N.ptr(out), ctypes.c_void_p(stream.cuda_stream)))
    return out[:n]


def _table_counts(table, queries):
    """Host int64[P]: how often each of the P query rows (uint64[P, W]) was drawn, 0 for a row the table does not
    hold.  A device table: the queries go up, one lookup, one gather of the multiplicities there, P counts come
    back.  A host table: the mirror."""
    q = np.ascontiguousarray(queries, np.uint64).reshape(-1, table.W)
    if not len(q):
        return np.zeros(0, np.int64)
    if _is_device_tensor(table.rows):
        import torch
        dev = table.rows.device
        with torch.cuda.device(dev):
            d_q = torch.from_numpy(q.view(np.int64)).to(dev)
            at = rows_find_device(table, d_q, len(q), torch.cuda.current_stream(dev)).to(torch.int64) & 0xFFFFFFFF
            hit = at != FIND_MISSING
            mult = table.mult.to(torch.int64) & 0xFFFFFFFF
            counts = torch.where(hit, mult[torch.where(hit, at, torch.zeros_like(at))], torch.zeros_like(at))
            return counts.cpu().numpy()
    d = min(int(table.length[0]), table.cap)
    at = rows_find_host(table.rows[:d], q)
    mult = np.concatenate([np.asarray(table.mult[:d], np.int64) & 0xFFFFFFFF, [0]])
    return mult[np.where(at == FIND_MISSING, d, at)]


# --- a weight per agent against a table (csrc/rows_price.inc) ------------------------------------------------
# Which panel of a table has the largest weight sum: the question both loops of the reference's column
# generation put to an ILP (xmin.py:229-290 with multiplicative weights, xmin.py:410-440 with the dual values),
# answered over panels that were drawn.  ``rows_score_host``, ``rows_price_host``, ``rows_mw_cover_host`` and
# ``rows_first_holder_host`` are the numpy contracts of csa_rows_price_async, csa_rows_mw_cover_async and
# csa_rows_first_holder_async, bit for bit.

PRICE_NONE = 0xFFFFFFFFFFFFFFFF
NO_ROW = 0xFFFFFFFF


def _price_input(rows, weights):
    p = np.ascontiguousarray(rows, np.uint64)
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    if p.ndim != 2:
        raise ValueError("rows must be uint64[n, W]")
    if not 0 < len(w) <= 64 * p.shape[1]:
        raise ValueError("%d weights do not fit rows of %d words" % (len(w), p.shape[1]))
    return p, w


def _member_columns(p, n):
    """bool[n, D]: column i = which rows hold agent i."""
    if not len(p):
        return np.zeros((n, 0), np.bool_)
    return np.ascontiguousarray(np.unpackbits(p.view(np.uint8), axis=1, bitorder="little")[:, :n].T).astype(np.bool_)


def _score_columns(cols, w):
    s = np.zeros(cols.shape[1], np.float64)
    with np.errstate(all="ignore"):
        for i in range(len(w)):
            np.add(s, w[i], out=s, where=cols[i])      # s = np.where(bit, s + w[i], s)
    return s


def rows_score_host(rows, weights):
    """float64[D]: per row the sum of ``weights[i]`` over its set bits i, from +0.0, one rounded add per member
    in ascending agent index -- rp_score_kernel's contract.  Agents 0..n-1 in turn over the whole column:
    ``s = np.where(bit, s + w[i], s)``."""
    p, w = _price_input(rows, weights)
    return _score_columns(_member_columns(p, len(w)), w)


def _best_of(sc):
    """(row, value) of the first maximum of the scores by ``>``, or (PRICE_NONE, -inf)."""
    if len(sc) and not np.isnan(sc).any():
        at = int(np.argmax(sc))                 # the first maximum
        return at, float(sc[at])
    at, value = PRICE_NONE, -np.inf
    for d in range(len(sc)):
        if at == PRICE_NONE or sc[d] > value:
            at, value = d, float(sc[d])
    return at, value


def rows_price_host(rows, weights, index_base=0, best=None):
    """csa_rows_price_async's contract: ``(index, value, scores)`` -- ``index_base`` + the row of the greatest
    score (compared as float64 values with >, ties to the lowest row) and that score; (PRICE_NONE, -inf) for
    an empty table.  ``best`` = a stored ``(index, value)``: CSA_PRICE_ACCUMULATE, the stored pair is replaced
    only by a strictly greater score, or when its index is PRICE_NONE."""
    sc = rows_score_host(rows, weights)
    at, value = _best_of(sc)
    if at != PRICE_NONE:
        at += int(index_base)
    if best is not None and (at == PRICE_NONE or not (int(best[0]) == PRICE_NONE or value > best[1])):
        at, value = int(best[0]), float(best[1])
    return at, value, sc


def weights_sum_host(weights, W):
    """The lane-strided sum of rp_round_kernel: the vector padded with +0.0 to 64 * W entries, its 64-wide
    rows added one after another from +0.0, then the 64 partial sums added left to right from +0.0."""
    wp = np.zeros(64 * W, np.float64)
    wp[:len(weights)] = weights
    partial = np.zeros(64, np.float64)
    for j in range(W):
        partial = partial + wp[64 * j:64 * j + 64]
    s = np.float64(0.0)
    for x in partial:
        s = s + x
    return s


def rows_mw_cover_host(rows, weights, chosen, rounds):
    """csa_rows_mw_cover_async's contract: ``rounds`` multiplicative-weights rounds over the table, from
    ``weights`` (float64[n]) and ``chosen`` (one flag per row).  Returns ``(picks int64[rounds], weights,
    chosen uint8[D], pick_scores float64[rounds])``, the inputs unchanged.  Per round, in the order of
    xmin.py:251-266: the best row p under the weights; its members' weights times 0.8; all weights times
    n / (their lane-strided sum); then, p chosen before: all weights 0.9 w + 0.1 (product and sum rounded
    apart), else p becomes chosen.  An empty table leaves the weights alone and picks NO_ROW."""
    p, w = _price_input(rows, weights)
    w = w.copy()
    n, W = len(w), p.shape[1]
    ch = np.array(chosen, np.uint8).reshape(-1).copy()
    if len(ch) != len(p):
        raise ValueError("one chosen flag per row")
    picks, ps = np.full(int(rounds), NO_ROW, np.int64), np.full(int(rounds), -np.inf, np.float64)
    cols = _member_columns(p, n)
    for r in range(int(rounds)):
        if not len(p):
            continue
        at, value = _best_of(_score_columns(cols, w))
        picks[r], ps[r] = at, value
        w = np.where(cols[:, at], w * 0.8, w)
        w = w * (np.float64(n) / weights_sum_host(w, W))
        if ch[at]:
            w = 0.9 * w + 0.1
        ch[at] = 1
    return picks, w, ch, ps


def rows_first_holder_host(rows, n):
    """int64[n]: the lowest row holding agent i, or NO_ROW -- csa_rows_first_holder_async's contract."""
    p = np.ascontiguousarray(rows, np.uint64)
    if p.ndim != 2 or not 0 < n <= 64 * p.shape[1]:
        raise ValueError("rows must be uint64[D, W] with 0 < n <= 64 W")
    if not len(p):
        return np.full(n, NO_ROW, np.int64)
    member = np.unpackbits(p.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
    return np.where(member.any(axis=0), member.argmax(axis=0), NO_ROW).astype(np.int64)


def rows_price_device(table, n, d_weights, stream, index_base=0, best=None, scores=False):
    """Enqueue csa_rows_price_async over RowTable ``table`` (its length read on the device) with the float64
    device tensor ``d_weights`` (host weights are uploaded on the stream) on ``stream``; nothing waits.  Returns
    ``(best, scores)``: int64[2] on the device -- ``index_base`` + the best row, the score's bits -- and the
    float64[cap] scores, or None unless ``scores``.  ``best`` given: CSA_PRICE_ACCUMULATE onto that tensor.  The
    scratch comes from torch's allocator on that stream."""
    import torch
    L = N.lib()
    dev = table.length.device
    with torch.cuda.stream(stream):
        if not _is_device_tensor(d_weights):
            d_weights = torch.from_numpy(np.ascontiguousarray(d_weights, np.float64)).to(dev)
        need = int(L.csa_rows_price_scratch_bytes(table.cap, table.W))
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        sc = torch.empty(max(table.cap, 1), dtype=torch.float64, device=dev) if scores else None
        flags = N.CSA_PRICE_ACCUMULATE if best is not None else 0
        if best is None:
            best = torch.empty(2, dtype=torch.int64, device=dev)
    N.check(L.csa_rows_price_async(N.ptr(table.rows), N.ptr(table.length), table.cap, table.W, int(n), N.ptr(d_weights),
                                   int(index_base), flags, N.ptr(sc), N.ptr(best), N.ptr(scratch), need,
                                   ctypes.c_void_p(stream.cuda_stream)))
    return best, sc


def rows_mw_cover_device(table, n, rounds, d_weights, d_chosen, stream, pick_scores=False):
    """Enqueue csa_rows_mw_cover_async: ``rounds`` rounds over RowTable ``table`` on ``stream``, 2 launches each,
    nothing waits.  ``d_weights`` (float64[n]) and ``d_chosen`` (uint8[cap]) are device tensors, read and
    written.  Returns ``(picks, pick scores)``: int32 of ``rounds`` uint32 words, and float64 or None."""
    import torch
    L = N.lib()
    dev = table.length.device
    rounds = int(rounds)
    with torch.cuda.stream(stream):
        need = int(L.csa_rows_price_scratch_bytes(table.cap, table.W))
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        picks = torch.empty(max(rounds, 1), dtype=torch.int32, device=dev)
        ps = torch.empty(max(rounds, 1), dtype=torch.float64, device=dev) if pick_scores else None
    N.check(L.csa_rows_mw_cover_async(N.ptr(table.rows), N.ptr(table.length), table.cap, table.W, int(n), rounds,
                                      N.ptr(d_weights), N.ptr(d_chosen), N.ptr(picks), N.ptr(ps), N.ptr(scratch), need,
                                      ctypes.c_void_p(stream.cuda_stream)))
    return picks[:rounds], (ps[:rounds] if pick_scores else None)


def rows_first_holder_device(table, n, stream):
    """Enqueue csa_rows_first_holder_async over RowTable ``table`` on ``stream``; nothing waits.  Returns an int32
    tensor of n uint32 words: the lowest row holding each agent, or NO_ROW."""
    import torch
    with torch.cuda.stream(stream):
        out = torch.empty(int(n), dtype=torch.int32, device=table.length.device)
    N.check(N.lib().csa_rows_first_holder_async(N.ptr(table.rows), N.ptr(table.length), table.cap, table.W, int(n),
                                                N.ptr(out), ctypes.c_void_p(stream.cuda_stream)))
    return out


# --- the maximin lottery over a table (csrc/rows_maximin.inc) -------------------------------------------------
# The reference's _dual_leximin_stage with no fixed probabilities and P ranging over drawn panels
# (xmin.py:293-321), as a zero-sum game solved by multiplicative weights: a lower bound (the lottery of the
# picks) and an upper bound (the weights as a dual point) on the optimum, no LP solver.  ``rows_maximin_host``
# is csa_rows_maximin_async's contract in numpy, bit for bit.

MaximinState = namedtuple("MaximinState", "weights scores cover row_count upper rounds best_row ratio")
MaximinState.__doc__ = """What csa_rows_maximin_async keeps between calls, on the host: ``weights`` float64[n],
``scores`` float64[D], ``cover`` int64[n], ``row_count`` int64[D], and the state block's four words -- ``upper``
(float), ``rounds`` done, ``best_row`` of the last fresh pass (PRICE_NONE for an empty table) and its ``ratio``
u."""

MaximinBuffers = namedtuple("MaximinBuffers", "weights scores cover row_count block")
MaximinBuffers.__doc__ = """The same state as device tensors: float64[n], float64[cap], int32[n] and int32[cap]
(uint32 words), int64[4] (the state block: bits of upper, rounds done, best row, bits of u)."""


def _maximin_arguments(n, W, rounds, shrink, resync):
    n, rounds, shrink, resync = int(n), int(rounds), float(shrink), int(resync)
    if not 0 < n <= 64 * W:
        raise ValueError("n = %d agents do not fit rows of %d words" % (n, W))
    if rounds < 0:
        raise ValueError("rounds must not be negative")
    if not 0.5 <= shrink < 1.0:
        raise ValueError("shrink = %r outside [0.5, 1)" % (shrink,))
    if not 1 <= resync <= 64:
        raise ValueError("resync = %d outside [1, 64]" % resync)
    return n, rounds, shrink, resync


def rows_maximin_host(rows, n, rounds, shrink=0.8, resync=16, state=None):
    """csa_rows_maximin_async's contract: ``(picks int64[rounds], MaximinState)``.  ``state=None`` starts
    (CSA_MAXIMIN_START): unit weights on the agents some row holds, +0.0 elsewhere, a score pass, ``upper`` = the
    best score / the lane-strided weight sum; a MaximinState continues it (the input is left unchanged).  Round r
    (0-based within the call): the first best row p of the scores is picked and counted, its members are
    covered once more and their weights become ``w * shrink`` with ``delta = w - w * shrink``; then, on a round
    that is not fresh, every row's score loses the sum of ``delta`` over its intersection with row p (ascending
    agent index from +0.0); on a fresh round -- ``(r + 1) % resync == 0`` or the call's last -- the weights are
    scaled by n / (their lane-strided sum), the scores are summed afresh, and ``upper`` falls to the best score /
    the new weights' sum when that is less.  An empty table picks NO_ROW and changes nothing."""
    p = np.ascontiguousarray(rows, np.uint64)
    if p.ndim != 2:
        raise ValueError("rows must be uint64[D, W]")
    D, W = p.shape
    n, rounds, shrink, resync = _maximin_arguments(n, W, rounds, shrink, resync)
    shrink = np.float64(shrink)
    cols = _member_columns(p, n)
    if state is None:
        w = np.where(cols.any(axis=1), 1.0, 0.0).astype(np.float64)
        cover, row_count, done = np.zeros(n, np.int64), np.zeros(D, np.int64), 0
        sc = _score_columns(cols, w)
        best_row, value = _best_of(sc)
        with np.errstate(all="ignore"):
            ratio = np.float64(np.inf) if best_row == PRICE_NONE else np.float64(value) / weights_sum_host(w, W)
        upper = ratio
    else:
        w, sc = np.array(state.weights, np.float64).reshape(-1), np.array(state.scores, np.float64).reshape(-1)
        cover, row_count = np.array(state.cover, np.int64).reshape(-1), np.array(state.row_count, np.int64).reshape(-1)
        if len(w) != n or len(cover) != n or len(sc) != D or len(row_count) != D:
            raise ValueError("the state is another table's")
        upper, done, best_row, ratio = np.float64(state.upper), int(state.rounds), int(state.best_row), np.float64(state.ratio)
    picks = np.full(rounds, NO_ROW, np.int64)
    with np.errstate(all="ignore"):
        for r in range(rounds if D else 0):
            at, _ = _best_of(sc)
            picks[r] = at
            row_count[at] += 1
            member = cols[:, at]
            cover[member] += 1
            done += 1
            v = w * shrink
            delta = np.where(member, w - v, 0.0)
            w = np.where(member, v, w)
            if (r + 1) % resync and r != rounds - 1:
                t = np.zeros(D, np.float64)
                for i in np.flatnonzero(member):
                    np.add(t, delta[i], out=t, where=cols[i])
                sc = sc - t
                continue
            w = w * (np.float64(n) / weights_sum_host(w, W))
            sc = _score_columns(cols, w)
            best_row, value = _best_of(sc)
            ratio = np.float64(value) / weights_sum_host(w, W)
            if ratio < upper:
                upper = ratio
    return picks, MaximinState(w, sc, cover, row_count, float(upper), done, best_row, float(ratio))


def rows_maximin_device(table, n, rounds, shrink=0.8, resync=16, state=None, stream=None):
    """Enqueue csa_rows_maximin_async over RowTable ``table`` on ``stream`` (default: the current stream of the
    table's device); nothing waits.  ``state=None`` starts on fresh buffers (CSA_MAXIMIN_START); a
    MaximinBuffers is continued in place.  Returns ``(picks, buffers)``: int32 of ``rounds`` uint32 words, and
    the MaximinBuffers.  Bad arguments raise ValueError here or CsaError from the library, before any launch."""
    import torch
    L = N.lib()
    dev = table.length.device
    n, rounds, shrink, resync = _maximin_arguments(n, table.W, rounds, shrink, resync)
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(stream):
        need = int(L.csa_rows_maximin_scratch_bytes(table.cap, table.W))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        picks = torch.empty(max(rounds, 1), dtype=torch.int32, device=dev)
        flags = 0
        if state is None:
            flags = N.CSA_MAXIMIN_START
            state = MaximinBuffers(torch.empty(n, dtype=torch.float64, device=dev),
                                   torch.empty(max(table.cap, 1), dtype=torch.float64, device=dev),
                                   torch.empty(n, dtype=torch.int32, device=dev),
                                   torch.empty(max(table.cap, 1), dtype=torch.int32, device=dev),
                                   torch.empty(4, dtype=torch.int64, device=dev))
    N.check(L.csa_rows_maximin_async(N.ptr(table.rows), N.ptr(table.length), table.cap, table.W, n, rounds, shrink,
                                     resync, flags, N.ptr(state.weights), N.ptr(state.scores), N.ptr(state.cover),
                                     N.ptr(state.row_count), N.ptr(state.block), N.ptr(picks), N.ptr(scratch), need,
                                     ctypes.c_void_p(stream.cuda_stream)))
    return picks[:rounds], state


def maximin_buffers_host(buffers, length):
    """A MaximinBuffers copied to the host as the MaximinState of a table of ``length`` rows (this waits)."""
    d = int(length)
    block = buffers.block.cpu().numpy().view(np.uint64)
    return MaximinState(buffers.weights.cpu().numpy(), buffers.scores[:d].cpu().numpy(),
                        buffers.cover.cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
                        buffers.row_count[:d].cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
                        float(block[0:1].view(np.float64)[0]), int(block[1]), int(block[2]),
                        float(block[3:4].view(np.float64)[0]))


class PanelMaximin:
    """The maximin lottery over a run's distinct panels after ``rounds`` multiplicative-weights rounds.

    ``panels``: the distinct picked panels (frozensets of agent ids) in ascending row order; ``rows``: their rows
    in the run's sorted table; ``counts``: how often each was picked (integers summing to ``rounds``);
    ``probabilities`` = counts / rounds.  ``alloc``: agent id -> ``Fraction(cover, rounds)``, the agent's exact
    selection probability under that lottery.  ``covered_agents``: the agents some drawn panel holds.
    ``lower``: a Fraction, the minimum of ``alloc`` over ``covered_agents`` -- a lower bound on the optimum of
    the maximin LP over the drawn panels, hence on LEXIMIN's minimum probability.  ``upper``: float, the least
    (best score / weight sum) over the fresh passes, an upper bound on the same optimum.  ``output_lines`` names
    the agents no drawn panel contains.  No rounds (or an empty run): no panels, ``lower`` = 0."""

    def __init__(self, picks, picked_rows, cover, covered, upper, n, agent_ids):
        from fractions import Fraction
        from .instance import unpack_panel
        ids = list(agent_ids)
        picks = [int(x) for x in np.asarray(picks, np.int64).tolist()]
        at = {}
        for r, p in enumerate(picks):
            if p != NO_ROW:
                at.setdefault(p, []).append(r)
        self.rows = sorted(at)
        self.counts = [len(at[p]) for p in self.rows]
        self.rounds = sum(self.counts)
        self.panels = [frozenset(ids[q] for q in unpack_panel(np.ascontiguousarray(picked_rows[at[p][0]]).view(np.uint64), n))
                       for p in self.rows]
        self.probabilities = [c / self.rounds for c in self.counts]
        cover = [int(x) for x in np.asarray(cover, np.int64).tolist()]
        self.alloc = {aid: Fraction(cover[i], self.rounds) if self.rounds else Fraction(0) for i, aid in enumerate(ids)}
        self.covered_agents = frozenset(ids[i] for i in range(n) if covered[i])
        self.lower = min((self.alloc[a] for a in self.covered_agents), default=Fraction(0))
        self.upper = float(upper)
        self.output_lines = ["Agent %s not contained in any drawn panel." % (aid,) for i, aid in enumerate(ids)
                             if not covered[i]]
        if len(self.covered_agents) == len(ids):
            self.output_lines.append("All agents are contained in some drawn panel.")

    def portfolio(self):
        """``(panels, probabilities)`` as ``portfolio_probabilities``, ``portfolio_composition`` and
        ``legacy_portfolio_overlap`` take them."""
        return list(self.panels), list(self.probabilities)

    def __eq__(self, other):
        return isinstance(other, PanelMaximin) and self.__dict__ == other.__dict__

    def __repr__(self):
        return "PanelMaximin(%d panels, %d rounds, lower=%s, upper=%r)" % (len(self.panels), self.rounds, self.lower,
                                                                          self.upper)


# --- the Nash-welfare lottery over a table (csrc/rows_nash.inc) -----------------------------------------------
# The lottery over drawn panels with the greatest product (geometric mean) of selection probabilities, by Cover's
# multiplicative iteration p_d <- p_d G_d / m, G_d = the sum of 1 / pi_i over row d, with the certificate
# GM(pi / s) <= optimum <= GM(pi / s) * (max G / m) * s.  ``rows_marginals_host`` and ``rows_nash_host`` are the
# contracts of csa_rows_marginals_async and csa_rows_nash_async in numpy, bit for bit.

NASH_TILE = 1024

NashState = namedtuple("NashState", "prob scores marginals ratio rounds best_row psum")
NashState.__doc__ = """What csa_rows_nash_async keeps between calls, on the host: ``prob`` float64[D] (p),
``scores`` float64[D] (G), ``marginals`` float64[n] (pi), and the state block's four words -- ``ratio`` (float:
(max G / m) * psum), ``rounds`` done, ``best_row`` (the first row holding max G; PRICE_NONE for an empty table) and
``psum`` (the ordered sum of p).  All belong to the same p."""

NashBuffers = namedtuple("NashBuffers", "prob scores marginals block")
NashBuffers.__doc__ = """The same state as device tensors: float64[cap], float64[cap], float64[n] and int64[4] (the
state block: bits of ratio, rounds done, best row, bits of psum)."""


def _nash_arguments(n, W, rounds):
    n, rounds = int(n), int(rounds)
    if not 0 < n <= 64 * W:
        raise ValueError("n = %d agents do not fit rows of %d words" % (n, W))
    if rounds < 0:
        raise ValueError("rounds must not be negative")
    return n, rounds


def _tile_marginals(member, prob):
    """member bool[D, n] (row-major), prob float64[D]: (pi, psum) in the marginal pass's order."""
    D, n = member.shape
    pi, psum = np.zeros(n, np.float64), np.float64(0.0)
    with np.errstate(all="ignore"):
        for t0 in range(0, D, NASH_TILE):
            part, ps = np.zeros(n, np.float64), np.float64(0.0)
            for d in range(t0, min(t0 + NASH_TILE, D)):
                np.add(part, prob[d], out=part, where=member[d])      # part = np.where(bit, part + p[d], part)
                ps = ps + prob[d]
            pi = pi + part
            psum = psum + ps
    return pi, psum


def rows_marginals_host(rows, prob, n):
    """csa_rows_marginals_async's contract: ``(pi float64[n], psum)`` -- agent i's selection probability under the
    lottery drawing row d with probability ``prob[d]``.  The rows are cut into tiles of 1024; within a tile every
    agent's sum runs from +0.0 in ascending row order, one rounded add per row that holds the agent (a row that
    does not adds nothing); the tiles' sums are added in ascending order from +0.0.  ``psum`` is the same
    two-level sum over all rows."""
    p = np.ascontiguousarray(rows, np.uint64)
    if p.ndim != 2 or not 0 < int(n) <= 64 * p.shape[1]:
        raise ValueError("rows must be uint64[D, W] with 0 < n <= 64 W")
    q = np.ascontiguousarray(prob, np.float64).reshape(-1)
    if len(q) != len(p):
        raise ValueError("one probability per row")
    pi, psum = _tile_marginals(np.ascontiguousarray(_member_columns(p, int(n)).T), q)
    return pi, float(psum)


def rows_nash_host(rows, n, rounds, mult=None, total=None, state=None):
    """csa_rows_nash_async's contract: a NashState after ``rounds`` more rounds.  ``state=None`` starts
    (CSA_NASH_START): ``p = mult / total`` (``mult`` one count per row, ``total`` defaulting to their sum; the
    run's own lottery) or, without ``mult``, ``1 / D``; a NashState continues it (the input is left unchanged).
    The pass: pi and psum as ``rows_marginals_host``; inv = 1 / pi for the m agents some row holds, +0.0
    elsewhere; G = the rows' sums of inv in ascending agent index; the best row = the first holding max G; ratio
    = (max G / m) * psum.  A round: p = p * (G / m), then the pass.  Every quotient is rounded before the product
    it feeds.  An empty table: (no rows, pi = +0.0, ratio = +inf, 0 rounds, PRICE_NONE, psum = +0.0); rounds change
    nothing.  Rows that hold nobody at all (m = 0) are outside the contract: the quotients by m give inf or NaN
    here as on the device."""
    p = np.ascontiguousarray(rows, np.uint64)
    if p.ndim != 2:
        raise ValueError("rows must be uint64[D, W]")
    D, W = p.shape
    n, rounds = _nash_arguments(n, W, rounds)
    cols = _member_columns(p, n)
    member = np.ascontiguousarray(cols.T)
    held = cols.any(axis=1)
    m = np.float64(int(held.sum()))

    def the_pass(prob):
        pi, psum = _tile_marginals(member, prob)
        inv = np.where(held, np.float64(1.0) / pi, 0.0)
        sc = _score_columns(cols, inv)
        at, value = _best_of(sc)
        return sc, pi, (np.float64(value) / m) * psum, at, psum

    with np.errstate(all="ignore"):
        if state is None:
            if mult is not None:
                mu = np.asarray(mult, np.int64).reshape(-1) & 0xFFFFFFFF
                if len(mu) != D:
                    raise ValueError("one multiplicity per row")
                total = int(mu.sum()) if total is None else int(total)
                if total <= 0:
                    raise ValueError("multiplicities with a total of 0")
                prob = mu.astype(np.float64) / np.float64(total)
            else:
                prob = np.full(D, np.float64(1.0) / np.float64(D) if D else 0.0, np.float64)
            if not D:
                return NashState(prob, np.zeros(0, np.float64), np.zeros(n, np.float64), float("inf"), 0, PRICE_NONE, 0.0)
            sc, pi, ratio, at, psum = the_pass(prob)
            done = 0
        else:
            prob, sc = np.array(state.prob, np.float64).reshape(-1), np.array(state.scores, np.float64).reshape(-1)
            pi = np.array(state.marginals, np.float64).reshape(-1)
            if len(prob) != D or len(sc) != D or len(pi) != n:
                raise ValueError("the state is another table's")
            ratio, done, at, psum = np.float64(state.ratio), int(state.rounds), int(state.best_row), np.float64(state.psum)
        for _ in range(rounds if D else 0):
            prob = prob * (sc / m)
            sc, pi, ratio, at, psum = the_pass(prob)
            done += 1
    return NashState(prob, sc, pi, float(ratio), done, at, float(psum))


def rows_marginals_device(table, n, d_prob, stream=None):
    """Enqueue csa_rows_marginals_async over RowTable ``table`` with the float64 device tensor ``d_prob`` (one
    entry per row of the table's capacity) on ``stream``; nothing waits.  Returns ``(pi, psum)``: float64[n] and
    float64[1] on the device."""
    import torch
    L = N.lib()
    dev = table.length.device
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(stream):
        need = int(L.csa_rows_marginals_scratch_bytes(table.cap, table.W))
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        pi = torch.empty(int(n), dtype=torch.float64, device=dev)
        psum = torch.empty(1, dtype=torch.float64, device=dev)
    N.check(L.csa_rows_marginals_async(N.ptr(table.rows), N.ptr(table.length), table.cap, table.W, int(n), N.ptr(d_prob),
                                       N.ptr(pi), N.ptr(psum), N.ptr(scratch), need, ctypes.c_void_p(stream.cuda_stream)))
    return pi, psum


def rows_nash_device(table, n, rounds, mult=None, total=None, state=None, stream=None):
    """Enqueue csa_rows_nash_async over RowTable ``table`` on ``stream`` (default: the current stream of the
    table's device); nothing waits.  ``state=None`` starts on fresh buffers (CSA_NASH_START) from ``mult`` (a
    device tensor of the table's uint32 multiplicity words, or host counts, which are uploaded) over ``total``, or
    uniformly without ``mult``; a NashBuffers is continued in place.  Returns the NashBuffers.  Bad arguments raise
    ValueError here or CsaError from the library, before any launch."""
    import torch
    L = N.lib()
    dev = table.length.device
    n, rounds = _nash_arguments(n, table.W, rounds)
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(stream):
        need = int(L.csa_rows_nash_scratch_bytes(table.cap, table.W))
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        flags, d_mult = 0, None
        if state is None:
            flags = N.CSA_NASH_START
            if mult is not None:
                if total is None:
                    raise ValueError("multiplicities on the device need their total")
                if not _is_device_tensor(mult):
                    mult = torch.from_numpy((np.asarray(mult, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(dev)
                d_mult = mult if mult.dtype == torch.int32 else mult.to(torch.int32)
                if d_mult.numel() < table.cap:
                    raise ValueError("one multiplicity per row of the table")
                if int(total) <= 0:
                    raise ValueError("multiplicities with a total of 0")
            state = NashBuffers(torch.empty(max(table.cap, 1), dtype=torch.float64, device=dev),
                                torch.empty(max(table.cap, 1), dtype=torch.float64, device=dev),
                                torch.empty(n, dtype=torch.float64, device=dev),
                                torch.empty(4, dtype=torch.int64, device=dev))
    N.check(L.csa_rows_nash_async(N.ptr(table.rows), N.ptr(table.length), table.cap, table.W, n, rounds, flags,
                                  N.ptr(d_mult), int(total or 0), N.ptr(state.prob), N.ptr(state.scores),
                                  N.ptr(state.marginals), N.ptr(state.block), N.ptr(scratch), need,
                                  ctypes.c_void_p(stream.cuda_stream)))
    return state


def nash_buffers_host(buffers, length):
    """A NashBuffers copied to the host as the NashState of a table of ``length`` rows (this waits)."""
    d = int(length)
    block = buffers.block.cpu().numpy().view(np.uint64)
    return NashState(buffers.prob[:d].cpu().numpy(), buffers.scores[:d].cpu().numpy(), buffers.marginals.cpu().numpy(),
                     float(block[0:1].view(np.float64)[0]), int(block[1]), int(block[2]),
                     float(block[3:4].view(np.float64)[0]))


def _geometric_mean(values):
    import math
    values = list(values)
    if not values or min(values) <= 0.0:
        return 0.0
    return math.exp(math.fsum(math.log(v) for v in values) / len(values))


class PanelNash:
    """The Nash-welfare lottery over a run's distinct panels after ``rounds`` rounds of Cover's iteration.

    ``probabilities``: float64[D], the lottery in the order of the run's sorted table (p / its sum).  ``alloc``:
    agent id -> that lottery's selection probability of the agent (float; 0.0 for an agent no drawn panel holds).
    ``covered_agents``: the agents some drawn panel holds; ``output_lines`` names the others.
    ``geometric_mean``: ``exp(fsum(log alloc) / m)`` over the covered agents -- a lower bound on the greatest
    geometric mean any lottery over the drawn panels reaches; ``gap``: the certificate (max G / m) * sum of p, at
    least 1 up to rounding; ``upper = geometric_mean * gap`` bounds that optimum from above.
    ``start_geometric_mean``: the same statistic at round 0 (LEGACY's own lottery over the drawn panels for
    ``start="legacy"``).  ``best_row`` / ``best_panel``: the row the next round would raise most (None and an
    empty set for an empty run).  An empty run: no probabilities, geometric means 0.0, gap and upper +inf."""

    def __init__(self, table, prob, marginals, psum, start_marginals, start_psum, ratio, rounds, best_row, n, ids):
        self._source, self._n, self._ids = table, int(n), list(ids)
        ids = self._ids
        prob = np.asarray(prob, np.float64)
        with np.errstate(all="ignore"):
            self.probabilities = prob / np.float64(psum) if len(prob) else prob.copy()
            pi = np.asarray(marginals, np.float64) / np.float64(psum) if len(prob) else np.zeros(n)
            pi0 = np.asarray(start_marginals, np.float64) / np.float64(start_psum) if len(prob) else np.zeros(n)
        covered = np.asarray(start_marginals, np.float64) != 0.0      # every start has full support
        self.alloc = {aid: float(pi[i]) for i, aid in enumerate(ids)}
        self.covered_agents = frozenset(ids[i] for i in range(n) if covered[i])
        self.geometric_mean = _geometric_mean(float(pi[i]) for i in range(n) if covered[i])
        self.start_geometric_mean = _geometric_mean(float(pi0[i]) for i in range(n) if covered[i])
        self.gap = float(ratio)
        self.upper = self.geometric_mean * self.gap if len(prob) else float("inf")
        self.rounds = int(rounds)
        self.best_row = None if int(best_row) == PRICE_NONE else int(best_row)
        self.best_panel = frozenset() if self.best_row is None else self._decode([self.best_row])[0]
        self.output_lines = ["Agent %s not contained in any drawn panel." % (aid,) for i, aid in enumerate(ids)
                             if not covered[i]]
        if len(self.covered_agents) == len(ids):
            self.output_lines.append("All agents are contained in some drawn panel.")

    def _decode(self, index):
        """The frozensets of the table's rows ``index``; only those rows are copied from a device table."""
        from .instance import unpack_panel
        t = self._source
        if not len(index):
            return []
        if _is_device_tensor(t.rows):
            import torch
            at = torch.as_tensor(np.asarray(index, np.int64), device=t.rows.device)
            words = t.rows.view(t.cap, t.W)[at].cpu().numpy()
        else:
            words = np.asarray(t.rows).view(np.int64).reshape(-1, t.W)[np.asarray(index, np.int64)]
        return [frozenset(self._ids[q] for q in unpack_panel(np.ascontiguousarray(r).view(np.uint64), self._n))
                for r in words]

    def portfolio(self, threshold=1e-9):
        """``(panels, probabilities)`` as ``portfolio_probabilities``, ``portfolio_composition`` and
        ``legacy_portfolio_overlap`` take them: the rows with probability >= ``threshold`` in table order, their
        probabilities divided by their ``fsum``.  Only the kept rows are decoded."""
        import math
        keep = np.flatnonzero(self.probabilities >= float(threshold))
        kept = [float(x) for x in self.probabilities[keep]]
        total = math.fsum(kept)
        return self._decode(keep), [x / total for x in kept]

    _FIELDS = ("alloc", "covered_agents", "geometric_mean", "start_geometric_mean", "gap", "upper", "rounds",
               "best_row", "best_panel", "output_lines")

    def __eq__(self, other):
        return isinstance(other, PanelNash) and all(getattr(self, f) == getattr(other, f) for f in self._FIELDS) and \
            np.array_equal(self.probabilities.view(np.uint64), other.probabilities.view(np.uint64))

    __hash__ = None

    def __getstate__(self):
        st = dict(self.__dict__)
        t = self._source
        if t is not None and _is_device_tensor(t.rows):       # pickles hold host arrays only
            rows = t.rows.view(t.cap, t.W).cpu().numpy().view(np.uint64)
            st["_source"] = RowTable(rows, None, None, np.array([t.cap], np.uint64), t.cap, t.W)
        elif t is not None:
            st["_source"] = RowTable(np.asarray(t.rows), None, None, np.asarray(t.length), t.cap, t.W)
        return st

    def __repr__(self):
        return "PanelNash(%d panels, %d rounds, geometric_mean=%r, gap=%r)" % (len(self.probabilities), self.rounds,
                                                                              self.geometric_mean, self.gap)


PanelPrice = namedtuple("PanelPrice", "panel value row first multiplicity")
PanelPrice.__doc__ = """The best distinct panel of a run under a weight per agent: ``panel`` (frozenset of agent
ids), ``value`` (its weight sum), ``row`` (its row in the run's sorted table), ``first`` (its lowest draw index)
and ``multiplicity``.  An empty run: (frozenset(), -inf, None, None, 0)."""


def weight_vector(weights, agent_ids):
    """float64[n] in the instance's agent order from a mapping agent id -> weight (KeyError for an agent it
    lacks) or a sequence of n weights; ValueError for another length or a weight that is not finite."""
    ids = list(agent_ids)
    if hasattr(weights, "keys"):
        w = np.array([weights[aid] for aid in ids], np.float64)
    else:
        w = np.array(weights, np.float64).reshape(-1)
        if len(w) != len(ids):
            raise ValueError("%d weights for %d agents" % (len(w), len(ids)))
    if not np.isfinite(w).all():
        raise ValueError("weights must be finite")
    return w


def _table_ops(table):
    """(operations, on the device?) for a RowTable: DeviceRowTables on its device's current stream, or
    HostRowTables."""
    if _is_device_tensor(table.rows):
        import torch
        dev = table.rows.device
        return DeviceRowTables(dev, torch.cuda.current_stream(dev)), True
    return HostRowTables(), False


def _rows_at(table, index, device):
    """The table's rows at ``index`` (clamped into the table: NO_ROW entries give some row, to be ignored),
    [len(index), W] as int64 words; nothing waits."""
    if device:
        at = (index.to(table.rows.dtype) & 0xFFFFFFFF).clamp(0, table.cap - 1)
        return table.rows.view(table.cap, table.W)[at]
    at = np.clip(np.asarray(index, np.int64) & 0xFFFFFFFF, 0, table.cap - 1)
    return np.asarray(table.rows).view(np.int64).reshape(-1, table.W)[at]


def committees_from_cover(picks, first_row, picked_rows, holder_rows, n, agent_ids):
    """The reference's return of _generate_initial_committees from a cover over a table: the picked rows are
    the committees of the multiplicative-weights stage; then, agents in order, each one no committee covers yet
    gets the lowest row holding it (which covers that row's members too), the counterpart of xmin.py:272-282.
    ``(committees, covered_agents, output_lines)``."""
    from .instance import unpack_panel
    committees, covered, lines = set(), set(), []
    decode = lambda row: frozenset(agent_ids[q] for q in unpack_panel(np.ascontiguousarray(row).view(np.uint64), n))
    seen = set()
    for r, p in enumerate(np.asarray(picks, np.int64).tolist()):
        if p != NO_ROW and p not in seen:
            seen.add(p)
            c = decode(picked_rows[r])
            committees.add(c)
            covered |= c
    for i, aid in enumerate(agent_ids):
        if aid in covered:
            continue
        if int(first_row[i]) == NO_ROW:
            lines.append("Agent %s not contained in any drawn panel." % (aid,))
            continue
        c = decode(holder_rows[i])
        committees.add(c)
        covered |= c
    if len(covered) == len(agent_ids):
        lines.append("All agents are contained in some drawn panel.")
    return committees, frozenset(covered), lines


class PanelComparison:
    """Two runs' panel tables side by side: the integers of a join's record (JOIN_RECORD) and the two runs'
    draws ``S_a`` / ``S_b``.  Every figure is one division of two exact integers, so the device's record and
    the host mirror's give the same floats.  With S = 0 on either side every figure is 0.0.

    ``shared``, ``only_a``, ``only_b``, ``union``: distinct panels drawn by both runs, by one alone, by either.
    """

    def __init__(self, record, S_a, S_b):
        self.record = [int(x) for x in record]
        self.S_a, self.S_b = int(S_a), int(S_b)
        self.union, self.shared, self.only_a, self.only_b = self.record[:4]

    def _over(self, num, den):
        return num / den if self.S_a and self.S_b and den else 0.0

    def jaccard(self):
        """Shared distinct panels over the union's."""
        return self._over(self.shared, self.union)

    def mass_a_on_b(self):
        """The share of run a's draws that fell on panels run b saw: the held-out coverage that b's Good-Turing
        ``coverage()`` predicts."""
        return self._over(self.record[6], self.S_a)

    def mass_b_on_a(self):
        return self._over(self.record[7], self.S_b)

    def overlap(self):
        """sum min(m_a / S_a, m_b / S_b) over the shared panels: 1 minus the total variation distance of the two
        empirical distributions."""
        return self._over(self.record[9], self.S_a * self.S_b)

    def total_variation(self):
        return 1 - self.overlap() if self.S_a and self.S_b else 0.0

    def cross_collision(self):
        """sum m_a m_b / (S_a S_b): the chance that a draw of a and a draw of b are one panel, an unbiased
        estimate of the sum of squared panel probabilities from independent samples -- beside
        ``collision_probability()``, the within-sample one."""
        return self._over(self.record[8], self.S_a * self.S_b)

    def __eq__(self, other):
        return isinstance(other, PanelComparison) and (self.record, self.S_a, self.S_b) == \
            (other.record, other.S_a, other.S_b)

    def __repr__(self):
        return "PanelComparison(shared=%d, only_a=%d, only_b=%d, S_a=%d, S_b=%d)" % (
            self.shared, self.only_a, self.only_b, self.S_a, self.S_b)


def _same_instance(a, b):
    if a._n != b._n or not (a._ids is b._ids or list(a._ids or ()) == list(b._ids or ())):
        raise ValueError("the two sides are over different instances (their agents differ)")


def compare_panel_distributions(a, b):
    """The PanelComparison of two PanelDistributions over one instance (two seeds of LEGACY: the reference's
    two-sample design, analysis.py:536-541, at the level of whole panels).  Both tables on one device: one
    csa_rows_join_async (select 0: the record alone) and one host copy of 15 words; otherwise the host mirror.
    The record's multiplicity sums must be the runs' S: RuntimeError otherwise.  ValueError for distributions
    over different instances; distributions that kept no panels raise PanelSet's message."""
    _same_instance(a, b)
    ta, tb = a.table(), b.table()
    if _is_device_tensor(ta.rows) and _is_device_tensor(tb.rows) and ta.rows.device == tb.rows.device:
        import torch
        dev = ta.rows.device
        with torch.cuda.device(dev):
            T = DeviceRowTables(dev, torch.cuda.current_stream(dev))
            j = T.join(ta, tb, 0, (a.S, b.S))
            head = torch.cat([T.status.view(torch.int64), j.record]).cpu().numpy()
        words = head[:2].view(np.uint32)
        record = [int(x) for x in head[2:].view(np.uint64)]
    else:
        host = lambda t: RowTable(*(x.cpu().numpy() if _is_device_tensor(x) else x for x in (t.rows, t.first, t.mult,
                                                                                          t.length)), t.cap, t.W)
        T = HostRowTables()
        j = T.join(host(ta), host(tb), 0, (a.S, b.S))
        words, record = T.status, j.record
    N.raise_status(words)
    if record[4] != a.S or record[5] != b.S:
        raise RuntimeError("panel comparison: the tables' multiplicities sum to %d and %d, the runs drew %d and %d"
                           % (record[4], record[5], a.S, b.S))
    return PanelComparison(record, a.S, b.S)


class PortfolioOverlap:
    """A LEGACY run beside a LEXIMIN / XMIN portfolio.  ``counts`` (int64[P]): how often the run drew each
    portfolio entry.  ``panels`` / ``panels_seen``: the portfolio's distinct panels, and those of them the run
    ever drew.  ``legacy_mass``: the share of the run's draws on the portfolio's panels.  ``portfolio_mass_seen``:
    the portfolio's probability on panels the run drew.  ``overlap``: sum over the distinct portfolio panels of
    min(m / S, w), w a panel's weights added up: 1 minus the total variation distance between the run's
    empirical distribution and the portfolio's."""

    def __init__(self, counts, panels, panels_seen, legacy_mass, portfolio_mass_seen, overlap, S):
        self.counts, self.panels, self.panels_seen, self.S = counts, int(panels), int(panels_seen), int(S)
        self.legacy_mass, self.portfolio_mass_seen, self.overlap = legacy_mass, portfolio_mass_seen, overlap


def portfolio_overlap(distribution, portfolio_rows, weights):
    """The PortfolioOverlap of a PanelDistribution and a portfolio given as packed rows uint64[P, W] with float64
    ``weights``.  One lookup of the P rows in the run's table and one gather of the multiplicities (on the
    device where the table is there; P counts are copied), then on the host in portfolio order, every float sum
    from ``0.`` by one float64 add per entry, left to right (as ``group_whist_host`` orders its sums):
    ``portfolio_mass_seen`` adds w_p over the entries with a non-zero count; an entry that repeats an earlier
    panel adds its weight to that panel's; ``overlap`` then adds min(m / S, w) over the distinct panels in
    the order of their first entry, and ``legacy_mass`` is the integer sum of their m over S.  S = 0: 0.0."""
    t = distribution.table()
    rows = np.ascontiguousarray(portfolio_rows, np.uint64).reshape(-1, t.W)
    w = np.ascontiguousarray(weights, np.float64).reshape(-1)
    if len(w) != len(rows):
        raise ValueError("one weight per portfolio panel")
    counts = _table_counts(t, rows)
    S = distribution.S
    slot, summed, mult = {}, [], []
    mass_seen = 0.
    for key, m, x in zip(map(bytes, rows), counts.tolist(), w.tolist()):
        if m:
            mass_seen += x
        e = slot.setdefault(key, len(summed))
        if e == len(summed):
            summed.append(x)
            mult.append(m)
        else:
            summed[e] += x
    overlap = 0.
    for m, x in zip(mult, summed):
        overlap += min(m / S, x) if S else 0.
    return PortfolioOverlap(counts, len(summed), sum(1 for m in mult if m), sum(mult) / S if S else 0.0, mass_seen,
                            overlap, S)


def composition_difference(a, b):
    """Two compositions over equal labels and k (CompositionHistogram or WeightedCompositionHistogram,
    either side: LEGACY against LEXIMIN, LEXIMIN against XMIN) compared group by group.  Returns a dict of
    "labels" and three float64[G] arrays: "total_variation", half the L1 distance between the two
    ``probabilities()`` rows; "mean" and "prob_absent", a's minus b's.  ValueError when the labels or
    k differ."""
    for h in (a, b):
        if not isinstance(h, (CompositionHistogram, WeightedCompositionHistogram)):
            raise ValueError("composition_difference takes two composition histograms")
    if a.labels != b.labels or a.k != b.k:
        raise ValueError("compositions over different groups or panel sizes")
    return {"labels": list(a.labels),
            "total_variation": 0.5 * np.abs(a.probabilities() - b.probabilities()).sum(axis=1),
            "mean": a.mean() - b.mean(),
            "prob_absent": a.prob_absent() - b.prob_absent()}


INTERSECTION_SHARES = ("population share", "panel share LEGACY", "panel share LEXIMIN", "pool share", "quota share")
# analysis.py:509-512, in the reference's order
INTERSECTION_DIFF_PAIRS = (("panel share LEXIMIN", "population share"), ("panel share LEGACY", "population share"),
                           ("panel share LEXIMIN", "pool share"), ("panel share LEGACY", "pool share"),
                           ("panel share LEXIMIN", "quota share"), ("panel share LEGACY", "quota share"),
                           ("panel share LEXIMIN", "panel share LEGACY"))


def intersectional_representation(instance, legacy_alloc, leximin_alloc, intersections):
    """The numbers of plot_intersectional_representation (analysis.py:474-530), without the plot.

    ``intersections``: a path to an ``intersections.csv``-shaped table, or rows
    ``((c1, f1), (c2, f2), population share)``.  Returns ``(table, errors)``: ``table`` maps
    "labels" to the ((c1, f1), (c2, f2)) pairs and each of INTERSECTION_SHARES to a float64 array in row
    order; ``errors`` maps the reference's seven (share 1, share 2) keys, in its order, to the mean
    squared difference.  The panel shares are the reference's float sums: the members' probabilities
    added in the allocation's own order from 0, divided by k.  A path that does not exist returns
    None, as the reference does; an unknown category or feature raises KeyError."""
    import os
    if isinstance(intersections, (str, os.PathLike)):
        if not os.path.exists(intersections):
            return None
        intersections = read_intersections(intersections)
    rows = [(tuple(a), tuple(b), float(share)) for a, b, share in intersections]
    enc = _encoding(instance)
    index = _feature_index(enc)
    member = _feature_membership(enc)
    pos = {aid: p for p, aid in enumerate(enc.agent_ids)}
    k, n = instance.k, len(instance.agents)
    allocs = []
    for alloc in (legacy_alloc, leximin_alloc):
        where = np.fromiter((pos[pers] for pers in alloc), np.int64, len(alloc))   # KeyError: not an agent
        allocs.append((where, list(alloc.values())))
    table = {name: np.zeros(len(rows), np.float64) for name in INTERSECTION_SHARES}
    table["labels"] = [(a, b) for a, b, _ in rows]
    for r, (a, b, share) in enumerate(rows):
        both = member[index(a)] & member[index(b)]
        table["population share"][r] = share
        for name, (where, probs) in zip(("panel share LEGACY", "panel share LEXIMIN"), allocs):
            table[name][r] = sum(probs[i] for i in np.flatnonzero(both[where]).tolist()) / k
        table["pool share"][r] = int(both.sum()) / n
        quota_share = 1
        for category, feature in (a, b):
            info = instance.categories[category][feature]
            quota_share *= ((info["min"] + info["max"]) / 2) / k
        table["quota share"][r] = quota_share
    errors = {}
    for s1, s2 in INTERSECTION_DIFF_PAIRS:
        d = table[s1] - table[s2]
        errors[(s1, s2)] = float(np.mean(d ** 2)) if len(rows) else float("nan")
    return table, errors
