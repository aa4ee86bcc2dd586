"""Drop-in for the LEGACY part of the reference's analysis.py, backed by HIP kernels.

Kept names and semantics (reference file:line):
  * ``Instance``, ``read_instance``    analysis.py:54-58, 108-138 (from .instance)
  * ``PairHistogram``                  analysis.py:68-98 -- same methods, backed by one
                                       packed array of the n(n-1)/2 pair values (row-major
                                       i < j) instead of a dict, filled on the device
  * ``legacy_find``                    analysis.py:141-159 -- restarts run on the device
  * ``legacy_probabilities``           analysis.py:162-191 -- the batch entry point:
                                       draw S panels (each panel's state in the registers
                                       of 1, 2 or 8 lanes of a wavefront, by instance
                                       shape), per-person counts, X^T X pair counts on fp4
                                       MFMA (exact 0/1 products, f32 accumulation; int8
                                       selectable), exact distinct-panel count; returns
                                       ``(alloc, found_panels, pair_histogram)``.
  * ``leximin_probabilities``,         analysis.py:194-228 -- the solver itself stays a host callable
    ``xmin_probabilities``             (``find_distribution=``, or the reference's module when
                                       importable); what follows it -- selection_probs, the pair
                                       histogram, the panel set -- is ``portfolio_probabilities``:
                                       one upload of the packed panels and the weights, the bit
                                       transpose, and portfolio_pairs_kernel, which sums every
                                       pair's and person's probabilities in portfolio order in
                                       float64, so the values are the reference's bit for bit.
  * ``leximin_composition``,           new: the same calls with a fourth result, the weighted group
    ``xmin_composition``,              composition of the portfolio (stats.WeightedCompositionHistogram) from
    ``portfolio_composition``          whist_count_kernel + whist_sum_kernel over the same upload -- float64
                                       sums in portfolio order, bit for bit stats.group_whist_host's.
  * ``legacy_panel_distribution``      new: ``legacy_probabilities`` with a fourth result, how often each
                                       distinct panel was drawn (stats.PanelDistribution) from uq_mult_kernel /
                                       unique_mult_kernel and mult_spectrum_kernel beside the distinct count.
  * ``legacy_panel_comparison``,       new: two runs (seeds 0 and 1, analysis.py:536-541) or a run and a portfolio
    ``legacy_portfolio_overlap``       side by side at the level of whole panels (stats.PanelComparison,
                                       stats.PortfolioOverlap), and ``PanelSet``'s set operators, from
                                       csa_rows_join_async / csa_rows_find_async over the sorted distinct rows.
The LEXIMIN / XMIN solvers (Gurobi) and the plotting code stay in the reference (CPU).
"""
import ctypes
import os
from collections import namedtuple
from typing import Dict, List, Tuple

import numpy as np

from . import _native as N
from .instance import Instance, read_instance, encode, encode_cached, unpack_panel  # noqa: F401
from . import legacy as _legacy
from .legacy import STREAM, seed, SelectionError, check_min_cats, mt_draw  # noqa: F401


def __getattr__(name):           # analysis.RNG_MODE follows legacy.RNG_MODE (set_rng_mode)
    if name == "RNG_MODE":
        return _legacy.RNG_MODE
    raise AttributeError(name)

ProbAllocation = Dict


def _divide(u, d):
    """u / d as the reference's `/` on every value (analysis.py:86-88): numpy true division, except
    integer counts over an int that float64 cannot hold exactly, which Python divides exactly
    (int / int is correctly rounded; numpy would round the divisor first)."""
    if u.dtype.kind in "iu" and isinstance(d, (int, np.integer)) and not isinstance(d, bool) and float(d) != d:
        return np.array([x / int(d) for x in u.tolist()], np.float64)
    return u / d


class PairHistogram:
    """analysis.py:68-98 with a packed backing store.

    The reference keeps a dict of the n(n-1)/2 pairs i < j in row-major key order
    (analysis.py:70); here the same values sit in one array ``_u`` of that length and
    order (strict upper triangle, row-major: pair (i, j) at i(n-1) - i(i-1)/2 + j-i-1).
    Integer counts stay exact until
    ``turn_into_probabilities_by_dividing_all_elements_by_given_number`` divides them
    (float64 true division, as the reference's ``/``).  A histogram built by
    ``legacy_probabilities`` keeps the device's n*n integer pair counts and materialises
    ``_u`` on first access: the triangle is packed and divided on the device
    (csa_pairs_upper_async) and only its n(n-1)/2 float64 values cross PCIe, so a caller
    that only reads per-person probabilities or ``len(found_panels)`` never moves it.
    A histogram built by ``portfolio_probabilities`` (LEXIMIN / XMIN) keeps the device's packed
    float64 triangle (``_dtri``) the same way: copied on first access, sorted on the device by
    ``stats.sorted_pair_probabilities``.  Pickles hold host data only.
    """

    _dtri = None    # device float64 triangle (portfolio_pairs_kernel's output), copied on first access

    def __init__(self, number_of_agents, uniform_distribution=False, counts=None):
        n = int(number_of_agents)
        self.n = n
        self._src = None        # lazily materialised integer counts: n*n numpy array or device tensor
        self._divs = []         # divisions pending on _src, applied in order at materialisation
        self._uv = None
        if counts is not None:
            if hasattr(counts, "device") and not isinstance(counts, np.ndarray):
                self._src = counts
            else:
                c = np.asarray(counts)
                assert c.shape == (n, n)
                self._src = c
        else:
            self._uv = np.zeros(n * (n - 1) // 2, np.int64)
        self._counts = self._S = None   # integer pair counts and S when built by finish()
        if uniform_distribution:
            npairs = n * (n - 1) // 2
            self._src = None
            self._uv = np.full(npairs, 1 / npairs if npairs else 0.0, np.float64)

    def _materialise_device(self):
        """Strict upper triangle of the device counts, packed (and divided by the first pending
        divisor) on the device; one n(n-1)/2 copy into pinned host memory."""
        import torch
        src, n = self._src, self.n
        m = n * (n - 1) // 2
        # the device divides only by a first divisor that is positive and exact in float64 (S, as
        # legacy_probabilities passes it); any other divisor -- negative, fractional types, huge ints --
        # is applied on the host, in order, as numpy true division
        d0 = self._divs[0] if self._divs else None
        on_device = d0 is not None and isinstance(d0, (int, float, np.integer, np.floating)) and \
            not isinstance(d0, bool) and float(d0) > 0.0 and float(d0) == d0
        div = float(d0) if on_device else 0.0
        rest = self._divs[1:] if on_device else list(self._divs)
        dt = torch.float64 if on_device else torch.int64
        dev = src.device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev)
            d = torch.empty(max(m, 1), dtype=dt, device=dev)
            N.check(N.lib().csa_pairs_upper_async(N.ptr(src), n, div, N.ptr(d), ctypes.c_void_p(st.cuda_stream)))
            h = torch.empty(max(m, 1), dtype=dt, pin_memory=True)
            h.copy_(d, non_blocking=True)
            st.synchronize()
        u = h.numpy()[:m]
        for dv in rest:
            u = _divide(u, dv)
        return u

    @classmethod
    def _from_device_triangle(cls, n, tri):
        """Histogram over a device float64 triangle (n(n-1)/2 values, at least one element allocated)."""
        h = cls(n)
        h._uv, h._dtri = None, tri
        return h

    def _materialise_triangle(self):
        """One copy of the device float64 triangle into pinned host memory; pending divisions follow."""
        import torch
        tri, m = self._dtri, self.n * (self.n - 1) // 2
        with torch.cuda.device(tri.device):
            st = torch.cuda.current_stream(tri.device)
            h = torch.empty(max(m, 1), dtype=torch.float64, pin_memory=True)
            h.copy_(tri[:max(m, 1)], non_blocking=True)
            st.synchronize()
        u = h.numpy()[:m]
        for dv in self._divs:
            u = _divide(u, dv)
        return u

    @property
    def _u(self):
        if self._uv is None:
            if self._dtri is not None:
                u = self._materialise_triangle()
                self._dtri = None
            elif isinstance(self._src, np.ndarray):
                u = self._src[np.triu_indices(self.n, 1)]
                for d in self._divs:
                    u = _divide(u, d)
            else:
                u = self._materialise_device()
            self._uv, self._src, self._divs = u, None, []
        return self._uv

    @_u.setter
    def _u(self, value):
        self._uv, self._src, self._divs, self._dtri = value, None, [], None

    def _index(self, i, j):
        return i * (self.n - 1) - i * (i - 1) // 2 + (j - i - 1)

    # dict-compatible accessors -----------------------------------------------------------
    def _key(self, key):
        i, j = sorted(key)
        if not (0 <= i < j < self.n):
            raise KeyError(key)
        return i, j

    def __getitem__(self, key):
        i, j = self._key(key)
        return self._u[self._index(i, j)].item()

    def _writable(self, as_float):
        u = self._u
        if as_float and u.dtype.kind != "f":
            u = u.astype(np.float64)
        elif not u.flags.writeable or u.base is not None:
            u = u.copy()
        self._u = u
        return u

    def __setitem__(self, key, value):
        i, j = self._key(key)
        self._counts = self._S = None
        self._writable(isinstance(value, float))[self._index(i, j)] = value

    def turn_into_probabilities_by_dividing_all_elements_by_given_number(self, num):
        # analysis.py:86-88 divides every value with Python's `/`: a zero divisor raises
        # ZeroDivisionError at once (for int and float values alike) when there is any pair
        if num == 0 and len(self):
            raise ZeroDivisionError("division by zero")
        if self._uv is None:
            self._divs.append(num)
        else:
            self._u = _divide(self._uv, num)
        self._counts = self._S = None

    def add_portfolio_of_panels_to_histogram(self, portfolio, probabilities, device=None):
        """analysis.py:90-95.  By default on the host, one ``np.add.at`` per panel.  ``device=True``
        adds float probabilities with portfolio_pairs_kernel onto the current values (the same
        float64 sums in the same order, so the same bits; the triangle then stays on the device
        until it is read).  Integer weights always take the host path, so counts stay ints."""
        self._counts = self._S = None
        if device:
            pairs = list(zip(portfolio, probabilities))
            if pairs and all(isinstance(pob, float) for _, pob in pairs):
                return self._add_portfolio_device(pairs)
            portfolio, probabilities = [p for p, _ in pairs], [w for _, w in pairs]
        for panel, pob in zip(portfolio, probabilities):
            idx = np.asarray(sorted(panel), np.int64)
            u = self._writable(isinstance(pob, float))
            ii, jj = np.triu_indices(len(idx), 1)
            np.add.at(u, self._index(idx[ii], idx[jj]), pob)

    def _add_portfolio_device(self, pairs):
        """``pairs``: (panel, float probability) in portfolio order; panels name agents 0..n-1, the
        histogram's keys.  The current values go to the device (or are there already) and
        portfolio_pairs_kernel adds onto them (CSA_PORTFOLIO_ACCUMULATE)."""
        import torch
        n = self.n
        rows = _pack_positions([panel for panel, _ in pairs], n)     # KeyError: a key outside 0..n-1
        weights = np.array([pob for _, pob in pairs], np.float64)
        m = n * (n - 1) // 2
        if self._dtri is not None and not self._divs and self._uv is None:
            tri = self._dtri
        else:
            tri = torch.from_numpy(np.ascontiguousarray(self._writable(True))).to("cuda") if m else \
                torch.zeros(1, dtype=torch.float64, device="cuda")
        _portfolio_launch(rows, weights, n, tri, None, accumulate=True)
        self._uv, self._src, self._divs, self._dtri = None, None, [], tri

    def upper(self):
        """Values of all pairs i < j in the reference's key order (row-major); read-only."""
        u = self._u.view()
        u.flags.writeable = False
        return u

    def get_dict(self):
        iu = np.triu_indices(self.n, 1)
        vals = self._u.tolist()
        return dict(zip(zip(iu[0].tolist(), iu[1].tolist()), vals))

    def __len__(self):
        return self.n * (self.n - 1) // 2

    def __getstate__(self):
        return {"n": self.n, "u": np.ascontiguousarray(self._u)}

    def __setstate__(self, st):
        self.n = st["n"]
        self._src, self._divs, self._uv = None, [], st.get("u")
        if self._uv is None:                     # round-4 pickles held the n*n matrix
            self._uv = np.asarray(st["m"])[np.triu_indices(self.n, 1)]
        self._counts = self._S = None


class PanelSet:
    """Set of distinct panels (found_panels, analysis.py:171,186), lazily materialised.

    ``len()`` is the device's exact distinct-panel count; iteration / membership
    decode the packed bitmasks (host array, or a device tensor sorted on the
    device, of which only the distinct rows are copied) into sorted agent-id
    tuples, as the reference's set holds them.  A sharded run keeps no panels:
    they are re-drawn where first read (``_redraw``).
    """

    def __init__(self, unique_count, packed=None, n=0, agent_ids=None):
        self._count = int(unique_count)
        self._packed = packed
        self._n = n
        self._ids = agent_ids
        self._set = None

    def __len__(self):
        return self._count

    _where = "panels were not kept; only len() is available"
    # a sharded run (distributed.PanelRedraw): nothing was kept or sent -- the job's panels are
    # re-drawn on this process's GPU when first read, then deduplicated like kept panels
    _redraw = None

    def _panels(self):
        """The kept (or re-drawn) panels, device tensor or host array; None if none were kept.  A re-draw
        that streams (distributed.PanelRedraw.table) leaves the distinct rows alone, already sorted and
        checked against the run's count: the job's S x W words exist nowhere."""
        if self._packed is None and self._redraw is not None:
            rd = self._redraw         # kept until the read has succeeded: a raised guard or count leaves it to retry
            if getattr(rd, "streams", None) is not None and rd.streams():
                self._packed, self._are_distinct = rd.table(self._count)[0], True
            else:
                self._packed, self._check_count = rd(), True
            self._redraw = None
        return self._packed

    def _device_distinct(self, p):
        """Sorted distinct rows of a device tensor of packed panels, as an int64[D, W] tensor on its device
        (csa_rows_sort_unique_async; one host wait, for the length).  The sorted length is a second exact
        count, independent of the hash-based one: it must equal len(self)."""
        import torch
        from .stats import rows_sort_unique_device
        if self._dev_rows is None:
            W = max((self._n + 63) // 64, 1)
            with torch.cuda.device(p.device):
                t = rows_sort_unique_device(p, p.numel() // W, W, torch.cuda.current_stream(p.device), lists=False)
                d = int(t.length.item())
            if d != self._count:
                raise RuntimeError("found_panels: the sorted panels hold %d distinct panels, the run counted %d"
                                   % (d, self._count))
            # a view keeps all S rows of the output alive: with duplicates only the D rows are kept
            self._dev_rows = t.rows if d == t.cap else t.rows[:d].clone()
        return self._dev_rows

    _dev_rows = None
    _are_distinct = False       # _packed holds distinct sorted host rows already

    def device_rows(self):
        """The distinct panels, sorted as ``rows()`` sorts them, as an int64[D, W] tensor on the device the
        kept panels are on; None when they are not on a device (not kept, host arrays, a sharded run)."""
        from .stats import _is_device_tensor
        if self._dev_rows is None and _is_device_tensor(self._packed):
            self._device_distinct(self._packed)
        return self._dev_rows

    def _distinct(self, p):
        """Sorted distinct rows of packed panels p; a re-drawn set must have the run's exact count.  Panels on
        a device are sorted there and only the distinct rows copied (CSA_ROWS_HOST=1: all of them, and
        np.unique on the host)."""
        from .stats import rows_host_path
        W = max((self._n + 63) // 64, 1)
        if hasattr(p, "device") and not isinstance(p, np.ndarray):
            if p.is_cuda and not rows_host_path():
                d = self._device_distinct(p)
                return np.ascontiguousarray(d.cpu().numpy()).view(np.uint64).reshape(-1, W)
            p = p.cpu().numpy()
        p = np.ascontiguousarray(p).view(np.uint64).reshape(-1, W)
        if self._are_distinct:
            return p
        rows = np.unique(p, axis=0) if len(p) else p
        if getattr(self, "_check_count", False) and len(rows) != self._count:
            raise RuntimeError("found_panels: the re-drawn panels hold %d distinct panels, the run counted %d"
                               % (len(rows), self._count))
        return rows

    def _materialise(self):
        if self._set is None:
            if self._panels() is None:
                raise RuntimeError(self._where)
            rows = self._distinct(self._packed)
            ids = self._ids
            self._set = {tuple(ids[q] for q in unpack_panel(r, self._n)) for r in rows}
            self._packed = None
        return self._set

    def __iter__(self):
        return iter(self._materialise())

    def __contains__(self, panel):
        return tuple(panel) in self._materialise()

    def __eq__(self, other):
        return set(self) == set(other)

    def rows(self):
        """The distinct panels as a host uint64[u, W] array (sorted rows), or None when the panels
        were not kept.  Of device panels the distinct rows are copied to the host here; a sharded run's
        are re-drawn (and deduplicated on the device as they are, where the re-draw streams)."""
        W = (self._n + 63) // 64
        if self._panels() is None:
            if self._set is None:
                return None
            pos = {aid: q for q, aid in enumerate(self._ids)}
            rows = np.zeros((len(self._set), max(W, 1)), np.uint64)
            for i, panel in enumerate(self._set):
                for aid in panel:
                    q = pos[aid]
                    rows[i, q >> 6] |= np.uint64(1) << np.uint64(q & 63)
            return np.unique(rows, axis=0) if len(rows) else rows
        self._packed = self._distinct(self._packed)   # keep the host rows (a re-draw happens once)
        self._check_count, self._are_distinct = False, True
        return self._packed

    # --- set algebra (the reference's found_panels is a Python set, printed beside LEXIMIN's and XMIN's,
    # analysis.py:575-582).  Two PanelSets of one instance whose distinct rows are on one device: one
    # csa_rows_join_async, the result's rows staying there.  Anything else -- host rows, unpickled sets,
    # different devices, a plain set / frozenset / iterable of agent-id tuples -- goes through the host mirror
    # (stats.rows_join_host) over rows().  Never through Python tuples.

    def _kept(self):
        if self._panels() is None and self._set is None:
            raise RuntimeError(self._where)

    def _pack_all(self, panels):
        """Agent-id tuples -> uint64[len, W] rows in the given order, as stats._pack_ids packs one; KeyError for
        an id that is no agent."""
        pos = {aid: q for q, aid in enumerate(self._ids)}
        panels = list(panels)
        rows = np.zeros((len(panels), max((self._n + 63) // 64, 1)), np.uint64)
        for i, panel in enumerate(panels):
            for aid in panel:
                q = pos[aid]
                rows[i, q >> 6] |= np.uint64(1) << np.uint64(q & 63)
        return rows

    def _pack(self, panels):
        """Agent-id tuples -> sorted distinct rows."""
        rows = self._pack_all(panels)
        return np.unique(rows, axis=0) if len(rows) else rows

    def _from_rows(self, rows, count, on_device):
        out = PanelSet(count, rows, self._n, self._ids)
        out._are_distinct = True
        if on_device:
            out._dev_rows = rows
        return out

    def _join(self, other, select, swap=False):
        """(record, result): the join's 11 integers and, with ``select``, the selected rows as a PanelSet.
        ``swap``: ``other`` is the left operand (the reflected operators)."""
        from . import stats as St
        self._kept()
        if isinstance(other, PanelSet):
            St._same_instance(self, other)
            other._kept()
            a, b = (other, self) if swap else (self, other)
            da, db = a.device_rows(), b.device_rows()
            if da is not None and db is not None and da.device == db.device and not St.rows_host_path():
                return self._join_device(da, db, select)
            ra, rb = a.rows(), b.rows()
        else:
            ra, rb = self.rows(), self._pack(other)
            if swap:
                ra, rb = rb, ra
        rows, _, _, count, record = St.rows_join_host((ra, None), (rb, None), select)
        return record, (self._from_rows(rows, count, False) if select else None)

    def _join_device(self, da, db, select):
        import torch
        from . import stats as St
        dev, W = da.device, max((self._n + 63) // 64, 1)
        with torch.cuda.device(dev):
            T = St.DeviceRowTables(dev, torch.cuda.current_stream(dev))
            ta, tb = (St.RowTable(d, None, None, torch.full((1,), d.shape[0], dtype=torch.int64, device=dev),
                                  d.shape[0], W) for d in (da, db))
            j = T.join(ta, tb, select, mults=False)
            head = torch.cat([T.status.view(torch.int64), j.length, j.record]).cpu().numpy()   # the one host wait
        N.raise_status(head[:2].view(np.uint32))
        record, count = [int(x) for x in head[3:].view(np.uint64)], int(head[2])
        if not select:
            return record, None
        rows = j.rows if count == j.cap else j.rows[:count].clone()     # a view would keep the whole output alive
        return record, self._from_rows(rows, count, True)

    def intersection(self, other):
        return self._join(other, 4)[1]

    def union(self, other):
        return self._join(other, 7)[1]

    def difference(self, other):
        return self._join(other, 1)[1]

    def symmetric_difference(self, other):
        return self._join(other, 3)[1]

    __and__, __or__, __sub__, __xor__ = intersection, union, difference, symmetric_difference
    __rand__, __ror__, __rxor__ = intersection, union, symmetric_difference

    def __rsub__(self, other):
        return self._join(other, 1, swap=True)[1]

    def isdisjoint(self, other):
        return self._join(other, 0)[0][1] == 0

    def issubset(self, other):
        return self._join(other, 0)[0][2] == 0

    def issuperset(self, other):
        return self._join(other, 0)[0][3] == 0

    __le__, __ge__ = issubset, issuperset

    def __lt__(self, other):
        record = self._join(other, 0)[0]
        return record[2] == 0 and record[3] > 0

    def __gt__(self, other):
        record = self._join(other, 0)[0]
        return record[3] == 0 and record[2] > 0

    def contains_many(self, panels):
        """bool[len(panels)]: which of the panels (agent-id tuples, any order, repeats allowed) are in the set
        -- one csa_rows_find_async over the sorted rows where they are on a device, its mirror otherwise."""
        from . import stats as St
        self._kept()
        W = max((self._n + 63) // 64, 1)
        q = self._pack_all(panels)
        d = self.device_rows()
        if d is None or St.rows_host_path() or not len(q):
            return St.rows_find_host(self.rows(), q) != St.FIND_MISSING
        import torch
        with torch.cuda.device(d.device):
            t = St.RowTable(d, None, None, torch.full((1,), d.shape[0], dtype=torch.int64, device=d.device), d.shape[0], W)
            at = St.rows_find_device(t, torch.from_numpy(q.view(np.int64)).to(d.device), len(q),
                                     torch.cuda.current_stream(d.device))
            return at.cpu().numpy().view(np.uint32) != St.FIND_MISSING

    # pickling (run_legacy_or_retrieve dumps the returned tuple, analysis.py:284-290): only host
    # data -- the distinct panels as packed rows (or the materialised set) -- so the pickle loads
    # on a machine without a GPU
    def __getstate__(self):
        st = {"count": self._count, "n": self._n, "ids": self._ids}
        if self._set is not None:
            st["set"] = self._set
        else:
            st["rows"] = self.rows()
        return st

    def __setstate__(self, st):
        self._count, self._n, self._ids = st["count"], st["n"], st["ids"]
        self._set = st.get("set")
        self._packed = st.get("rows")


def _with_address(enc, columns_data, check_same_address_columns):
    """Same-address rings for the encoded agents (None without columns)."""
    if columns_data is None or not check_same_address_columns:
        return None
    return _legacy.address_rings(enc.agent_ids, columns_data, check_same_address_columns)


def _address_request(instance, columns_data, check_same_address_columns, devices=None):
    """The household keywords of a Monte Carlo call, checked before anything touches the device: None
    without them, else ``(columns_data, check_same_address_columns)``.  ValueError for one keyword without
    the other, for columns that are not an (address, zip) pair, for an agent without them, and for what a
    household-aware run is not offered with: a world of more than one rank, and ``devices=``."""
    if columns_data is None and check_same_address_columns is None:
        return None
    if columns_data is None or check_same_address_columns is None:
        raise ValueError("columns_data and check_same_address_columns go together")
    cols = list(check_same_address_columns)
    if len(cols) != 2:
        raise ValueError("check_same_address_columns names two columns (address, zip), got %d" % len(cols))
    for aid in instance.agents:
        row = columns_data.get(aid)
        if row is None or cols[0] not in row or cols[1] not in row:
            raise ValueError("columns_data has no %s / %s for agent %r" % (cols[0], cols[1], aid))
    from . import distributed as D
    if D.world_size() > 1:
        raise ValueError("check_same_address_columns: sharded runs (world size %d) are not offered; run on one "
                         "process" % D.world_size())
    if devices is not None:
        raise ValueError("check_same_address_columns: devices= is not offered; run on one device")
    return columns_data, cols


class _Households:
    """For the span of one Philox run: the instance's handle carries the address rings and draws its
    batches on the household kernels (CSA_ADDRESS_BATCH).  Both are taken away on exit -- after the run's one
    host wait, because csa_instance_set_address frees device memory."""

    def __init__(self, enc, ring):
        self.enc, self.ring = enc, ring

    def __enter__(self):
        L = N.lib()
        N.check(L.csa_instance_set_address(self.enc.handle, N.ptr(self.ring)))
        N.check(L.csa_instance_set_address_route(self.enc.handle, N.CSA_ADDRESS_BATCH))

    def __exit__(self, *exc):
        L = N.lib()
        rc = L.csa_instance_set_address(self.enc.handle, None)
        N.check(L.csa_instance_set_address_route(self.enc.handle, N.CSA_ADDRESS_GENERAL))
        if exc[0] is None:
            N.check(rc)


def legacy_find(feature_info, agents, k, rng: str = None, *, columns_data=None,
                check_same_address_columns=None) -> List:
    """analysis.py:141-159: one accepted panel, pick order, restarts on the device (Philox
    stream) or, with rng="mt" (default: legacy.RNG_MODE), on the host from the stdlib random
    stream as the reference consumes it.  With ``columns_data`` and
    ``check_same_address_columns`` the draws delete same-address people (legacy.py:109-113;
    the reference's legacy_find always passes check_same_address=False, analysis.py:150-151)."""
    return legacy_find_batch(feature_info, agents, k, 1, rng=rng, columns_data=columns_data,
                             check_same_address_columns=check_same_address_columns)[0]


def legacy_find_batch(feature_info, agents, k, count, max_attempts=0, rng: str = None, *, columns_data=None,
                      check_same_address_columns=None):
    """``count`` consecutive legacy_find calls in one launch (XMIN's caller, xmin.py:464-474)."""
    enc = encode_cached(feature_info, agents)
    k = int(k)
    ring = _with_address(enc, columns_data, check_same_address_columns)
    ids = enc.agent_ids
    if (rng or _legacy.RNG_MODE) == "mt":
        picks, _, _ = mt_draw(enc, k, int(count), max_attempts=max_attempts, addr_next=ring)
        return [[ids[int(p)] for p in row[:k] if p >= 0] for row in picks]
    picks = np.full((int(count), max(k, 1)), -1, np.int32)
    L = N.lib()
    first = STREAM.take_panels(count)
    if ring is not None:
        N.check(L.csa_instance_set_address(enc.handle, N.ptr(ring)))
    try:
        N.check(L.csa_legacy_find(enc.handle, k, STREAM.key, first, int(count), max_attempts, N.ptr(picks), None))
    finally:
        if ring is not None:
            N.check(L.csa_instance_set_address(enc.handle, None))
    return [[ids[int(p)] for p in row[:k] if p >= 0] for row in picks]


class LegacyRaw:
    """Integer results of one legacy_probabilities run (exact, before division).  ``stats``: the
    run's draw statistics (attempts, SelectionErrors, min-quota rejections; see draw_stats)."""

    def __init__(self, counts, pairs, unique, panels, attempts, stats=None, composition=None, multiplicity=None):
        self.counts, self.pairs, self.unique, self.panels, self.attempts = counts, pairs, unique, panels, attempts
        self.stats = stats
        self.composition = composition     # host int64[G, k + 1] when the run was given groups
        # when the run was asked for multiplicities: (first, mult) device lists of `unique` uint32 words,
        # the host spectrum and the sum of the squared multiplicities
        self.multiplicity = multiplicity


STAT_KEYS = ("attempts", "selection_errors", "rejections")
# draw statistics of the last legacy_probabilities call (SURVEY.md section 5 "Metrics"): the
# reference prints "Rejected" per min-quota rejection (analysis.py:159) and restarts silently on a
# SelectionError (analysis.py:152-153); here both are counted on the device
LAST_RUN_STATS = None


def reset_draw_stats(enc, stream=None):
    """Zero the instance's draw statistics before a batch: ordered on ``stream`` (a torch stream the
    batch's draws run on; no host wait), or, without one, after the instance's own streams and the
    streams of the encoding's cached DevicePipeline (its draw stream included: draws a caller
    enqueued there may still be counting) are idle (csa_instance_draw_stats_reset) -- never a
    device-wide synchronisation.  A caller that drew on streams of its own (bench.py)
    synchronises them first or passes the stream."""
    if stream is None:
        pipe = getattr(enc, "_pipe", None)
        for st in (getattr(pipe, "draw_stream", None), getattr(pipe, "stream", None)):
            if st is not None:
                st.synchronize()
    N.check(N.lib().csa_instance_draw_stats_reset(enc.handle, ctypes.c_void_p(stream.cuda_stream)
                                                  if stream is not None else None))


def draw_stats(enc, reset=False):
    """Totals of the instance's draws since creation / the last reset (csa_instance_draw_stats):
    {"attempts", "selection_errors", "rejections"}.  Synchronises the device."""
    out = np.zeros(3, np.uint64)
    N.check(N.lib().csa_instance_draw_stats(enc.handle, 1 if reset else 0, N.ptr(out)))
    return dict(zip(STAT_KEYS, (int(x) for x in out)))


def legacy_sample_raw(enc, k, iterations, random_seed, panel_begin=0, want_pairs=True, want_panels=True,
                      want_attempts=False, max_attempts=0, devices=None):
    """Run the whole batch through csa_legacy_sample and return integer results.  ``devices``
    (a list of HIP device ids, repeats allowed) shards the panels over those devices of this
    process through csa_legacy_sample_devices; the results are identical."""
    S = int(iterations)
    flags = N.CSA_WANT_COUNTS | N.CSA_WANT_UNIQUE
    counts = np.zeros(enc.n, np.int64)
    pairs = np.zeros((enc.n, enc.n), np.int64) if want_pairs else None
    panels = np.zeros((S, enc.W), np.uint64) if want_panels else None
    attempts = np.zeros(S, np.uint32) if want_attempts else None
    unique = np.zeros(1, np.uint64)
    if want_pairs:
        flags |= N.CSA_WANT_PAIRS
    if want_panels:
        flags |= N.CSA_WANT_PANELS
    seed64 = int(random_seed) & 0xFFFFFFFFFFFFFFFF
    outs = (N.ptr(panels), N.ptr(counts), N.ptr(pairs), N.ptr(unique), N.ptr(attempts))
    reset_draw_stats(enc)
    if devices is None:
        rc = N.lib().csa_legacy_sample(enc.handle, int(k), seed64, panel_begin, S, flags, max_attempts, *outs)
    else:
        dev = np.ascontiguousarray(devices, np.int32)
        rc = N.lib().csa_legacy_sample_devices(enc.handle, N.ptr(dev), len(dev), int(k), seed64, panel_begin, S,
                                               flags, max_attempts, *outs)
    if rc == N.CSA_E_BAD_QUOTAS:
        raise AssertionError(N.last_error())     # analysis.py:174-176
    if rc == N.CSA_E_NO_CANDIDATE:
        raise KeyError("")                       # legacy.py:188
    N.check(rc)
    return LegacyRaw(counts, pairs, int(unique[0]), panels, attempts, draw_stats(enc))


def cached_pipeline(enc, k, chunk):
    """The encoding's DevicePipeline for draws of at most ``chunk`` panels per launch on the current
    device (picks / XT / pair scratch sized to one chunk, reused across calls; no n*n pair matrix of
    its own -- callers pass a fresh one per call).  Rebuilt when k, the device or a larger chunk
    asks for it."""
    import torch
    from .device import DevicePipeline
    pipe = getattr(enc, "_pipe", None)
    dev = torch.device("cuda", torch.cuda.current_device())
    if pipe is None or pipe.max_panels < int(chunk) or pipe.k != int(k) or pipe.device != dev:
        enc._pipe = None                      # release the old buffers before allocating new ones
        pipe = enc._pipe = DevicePipeline(enc, k, int(chunk), want_pairs=True, want_unique=True, pairs_buffer=False,
                                          device=dev)
    return pipe


def read_draw_stats(enc, out, stream):
    """The instance's draw statistics into ``out`` (three int64 device words), ordered on ``stream``: no host wait."""
    N.check(N.lib().csa_instance_draw_stats_async(enc.handle, N.ptr(out), ctypes.c_void_p(stream.cuda_stream)))


def distinct_table(enc, S, dev):
    """The encoding's cached distinct-count table (distributed.HashTable), grown to hold S panels.  A batch takes it
    BEFORE its draws: allocated on the pipeline stream, which the draw stream waits on, and the side stream on that."""
    table = getattr(enc, "_table", None)
    if table is None or table.device != dev:
        from .distributed import HashTable
        table = enc._table = HashTable(S, dev)
    table.ensure(S)
    return table


def enqueue_group_hist(groups, d_masks, panels, S, W, k, status, stream):
    """group_hist_kernel over a batch's S device panels on ``stream``, into a zeroed int64[G, k + 1] table (made on
    that stream; at least one element, so G = 0 still has something to reduce and copy).  Returns the flat table;
    errors land in ``status``.  ``d_masks``: ``groups.device_masks(device, W)``."""
    import torch
    from .stats import group_hist_device
    with torch.cuda.stream(stream):
        d_hist = torch.zeros(max(len(groups) * (k + 1), 1), dtype=torch.int64, device=panels.device)
    group_hist_device(panels, S, W, d_masks, len(groups), k + 1, d_hist, status, stream)
    return d_hist


def legacy_sample_device(enc, k, S, random_seed, keep_panels=True, chunk=1 << 20, host_panels=None,
                         host_stats=None, groups=None, multiplicity=False):
    """One legacy_probabilities batch on the device through a DevicePipeline cached with the
    encoding (picks / XT / scratch buffers reused across calls).  Panels and hashes of the whole
    batch go to fresh device tensors (the exact distinct count needs all of them; with
    ``keep_panels`` the returned PanelSet keeps the panel tensor and decodes it only when
    iterated).  Returns LegacyRaw with host counts and device pair counts (PairHistogram
    materialises them lazily).  ``host_panels`` (uint64[S, W], MT mode: drawn on the host)
    replaces the device draw; the counting, pairs and distinct count still run on the device
    (``host_stats``: that draw's statistics).  ``groups`` (a stats.GroupSet): group_hist_kernel also
    runs over the batch's panels, after the draws, on the stream of the distinct count -- beside the
    counting and pairs with device draws -- and its int64[G, k + 1] table comes back in the same host
    copy (``LegacyRaw.composition``); its status lands in the same status block.  ``multiplicity``:
    csa_unique_mult_async and csa_mult_spectrum_async (4096 bins) follow the distinct count on its stream;
    the list's length, the spectrum and the summary words ride in the same host copy, the (first,
    multiplicity) lists stay on the device (``LegacyRaw.multiplicity``).  Only a spectrum that overflows
    the 4096 bins costs a second pass and copy."""
    import torch
    S, k = int(S), int(k)
    C = max(1, min(S, int(chunk)))
    pipe = cached_pipeline(enc, k, C)
    W = enc.W
    dev = pipe.device
    with torch.cuda.device(dev), torch.cuda.stream(pipe.stream):
        panels = torch.empty(max(S * W, 1), dtype=torch.int64, device=dev)
        hashes = torch.empty(max(2 * S, 2), dtype=torch.int64, device=dev)
        pairs = torch.empty(enc.n * enc.n, dtype=torch.int64, device=dev)
        # status before the draws; the counters after the draws are enqueued (the draw stream does not
        # wait for them, the counting on this stream does).  A one-chunk call folds the status and
        # statistics resets into its draw call (csa_draw_xt_async).
        one = host_panels is None and 0 < S <= C and os.environ.get("CSA_DRAW_XT", "1") != "0"
        pipe.reset(pairs=False, counts=host_panels is not None, status=not one)
        if host_panels is None and not one:
            reset_draw_stats(enc, pipe.stream)
        table = distinct_table(enc, S, dev)
        d_masks = groups.device_masks(dev, W) if groups is not None else None
        drawn = None  # what the distinct count's side stream waits for: the draws
        with pipe.bound(panels=pipe.panels, hashes=pipe.hashes, pairs=pairs):
            if one:
                # one chunk: draw on the pipeline stream; draw_lane_kernel's fused pack also writes the XT
                # blocks (csa_draw_xt_async), so the counting is the pair kernel alone and the counts
                # are the pair diagonal -- the transpose pass leaves the call's serial tail
                pipe.panels, pipe.hashes = panels[:S * W], hashes[:2 * S]
                xt_done = pipe.draw_xt(random_seed, 0, S, reset=True)
                drawn = pipe.stream.record_event()
                if not xt_done:
                    pipe.counts.zero_()
                    pipe.transpose_count(S)
                pipe.pair_counts(S, overwrite=True, alone=True)
                if xt_done:
                    pipe.counts_from_pairs()
            elif host_panels is None:
                # chunk draws on the pipeline's draw stream, counting and pairs on its stream, overlapped
                # (DevicePipeline.draw_count_chunks); two draw streams were measured slower
                # (profiles/r04f_draw_streams/)
                pipe.draw_count_chunks(random_seed, 0, S, panels, hashes, C, overwrite_pairs=True, reset_counts=True)
                drawn = pipe.draw_stream.record_event()
            else:
                for off in range(0, S, C):
                    ln = min(C, S - off)
                    pipe.panels, pipe.hashes = panels[off * W:(off + ln) * W], hashes[2 * off:2 * (off + ln)]
                    src = np.ascontiguousarray(host_panels[off:off + ln], np.uint64).view(np.int64).reshape(-1)
                    pipe.panels.copy_(torch.from_numpy(src), non_blocking=False)
                    pipe.hash(ln)
                    pipe.transpose_count(ln)
                    pipe.pair_counts(ln, overwrite=off == 0)
        if S == 0:
            pairs.zero_()
        # the group histogram and the multiplicity passes ride on the distinct count's stream, before its hand-back
        ust = pipe.distinct_count(table, hashes, panels, S, drawn)
        if groups is not None:
            d_hist = enqueue_group_hist(groups, d_masks, panels, S, W, k, pipe.status, ust)
        if multiplicity:
            from .stats import unique_mult_device
            m_first, m_mult, m_out = unique_mult_device(hashes, panels, S, W, pipe.status, ust, MULT_BINS)
        pipe.rejoin(ust)
        # counts, distinct count, draw statistics and status in ONE copy: the call's one host wait
        fields = [("counts", pipe.counts), ("unique", table.count)]
        if host_panels is None:
            st_d = torch.zeros(3, dtype=torch.int64, device=dev)
            read_draw_stats(enc, st_d, pipe.stream)
            fields.append(("stats", st_d))
        if multiplicity:
            fields += zip(MULT_FIELDS, m_out.split([1, MULT_BINS, 4]))
        if groups is not None:
            fields.append(("hist", d_hist))
        h, status = pipe.host_fields(fields)
        N.raise_status(status)
        counts = h["counts"].copy()
        unique = int(h["unique"][0])
        stats = dict(zip(STAT_KEYS, (int(x) for x in h["stats"]))) if host_panels is None else host_stats
        comp = h["hist"][:len(groups) * (k + 1)].reshape(len(groups), k + 1).copy() if groups is not None else None
        mult = _multiplicity(h, m_first, m_mult, S, unique, pipe.stream) if multiplicity else None
    return LegacyRaw(counts, pairs.view(enc.n, enc.n), unique, panels[: S * W] if keep_panels else None, None,
                     stats, comp, mult)


MULT_BINS = 4096   # spectrum bins of a multiplicity run's first pass; a longer tail takes a second one
# stats.unique_mult_device's output record: [list length | spectrum[bins] | overflow, max, sum m^2, sum m]
MULT_FIELDS = ("mult_length", "mult_spectrum", "mult_sums")


def _multiplicity(h, d_first, d_mult, S, unique, stream):
    """LegacyRaw.multiplicity from the host copy ``h`` of unique_mult_device's record (MULT_FIELDS) and the
    device lists.  The list must be as long as the distinct count and its multiplicities must sum to S; a
    spectrum beyond MULT_BINS is taken again with max + 1 bins."""
    import torch
    length, spectrum, sums = (h[f] for f in MULT_FIELDS)
    distinct, (over, top, sq, total) = int(length[0]), (int(x) for x in sums)
    if distinct != unique or total != S:
        raise RuntimeError("panel multiplicities: %d list entries summing to %d, the run counted %d distinct panels "
                           "in %d draws" % (distinct, total, unique, S))
    if over:
        with torch.cuda.stream(stream):
            out = torch.empty(1 + top + 1 + 4, dtype=torch.int64, device=d_mult.device)
            d_len, d_spectrum, d_sums = out.split([1, top + 1, 4])
            d_len[:] = distinct
            N.check(N.lib().csa_mult_spectrum_async(N.ptr(d_mult), N.ptr(out), S, N.ptr(d_spectrum), top + 1,
                                                    N.ptr(d_sums), ctypes.c_void_p(stream.cuda_stream)))
            _, spectrum, again = (t.numpy() for t in out.cpu().split([1, top + 1, 4]))
        if again[0] or int(again[3]) != S:
            raise RuntimeError("panel multiplicities: the spectrum's second pass disagrees with its first")
    return {"first": d_first[:distinct], "mult": d_mult[:distinct], "spectrum": spectrum[:top + 1].copy(),
            "sum_squares": sq}


def legacy_probabilities(instance: Instance, iterations: int, random_seed: int,
                         keep_panels: bool = True, rng: str = None,
                         devices=None, *, columns_data=None,
                         check_same_address_columns=None) -> Tuple[ProbAllocation, PanelSet, PairHistogram]:
    """analysis.py:162-191 on the GPU.

    Returns ``({agent_id: count/S}, found_panels, pair_histogram)`` with the
    pair histogram divided by S, as the reference.  With torch.distributed
    initialised and world size > 1 the panels are sharded over ranks (see
    ``distributed.legacy_probabilities_distributed``).

    ``rng="mt"`` (default: ``legacy.RNG_MODE``) reproduces the reference's own
    stream: ``random.seed(random_seed)`` (analysis.py:169), then the panels are
    drawn on the host from the stdlib MT19937 state exactly as legacy.py:149
    consumes it (csa_legacy_draw_mt) and counted / paired / deduplicated on the
    device.  It matches the published reference_output probabilities.

    ``devices`` (Philox mode, one process): shard the panels over these HIP
    devices through csa_legacy_sample_devices instead of torch.distributed.

    A sharded run's found_panels hold no panels: reading them on any rank re-draws the job's panels
    on that rank's GPU (``distributed.PanelRedraw``), without a collective.

    ``columns_data`` and ``check_same_address_columns`` (as ``legacy_find`` takes them) make the run
    household-aware: every pick also removes the people still in the pool at the pick's address
    (check_same_address, legacy.py:78-113), so no panel holds two members of a household.  In Philox mode
    the batches run on the household forms of the register kernels where the instance fits them
    (CSA_ADDRESS_BATCH), on draw_kernel<64, ..., true> otherwise; ``rng="mt"`` passes the rings to the host
    draw.  One process and one device: with the keywords, a world of more than one rank and ``devices=``
    raise ValueError before anything runs.  ``legacy_composition``, ``legacy_panel_distribution``,
    ``legacy_panel_comparison``, ``legacy_initial_committees``, ``legacy_maximin`` and ``legacy_nash`` take the same
    keywords; ``legacy_price``, ``run_legacy_or_retrieve`` and the cache do not.
    """
    address = _address_request(instance, columns_data, check_same_address_columns, devices)
    return _legacy_run(instance, iterations, random_seed, keep_panels, rng, devices, None, address=address)[:3]


# what one LEGACY run gives, the public calls take their slice: composition (a stats.CompositionHistogram) for a
# run given groups, distribution (a stats.PanelDistribution) for one asked for multiplicities, None otherwise
LegacyRun = namedtuple("LegacyRun", "alloc panels histogram composition distribution", defaults=(None, None))


def _legacy_run(instance, iterations, random_seed, keep_panels, rng, devices, groups, multiplicity=False,
                address=None):
    """legacy_probabilities' body, returning a LegacyRun; with ``groups`` (a stats.GroupSet) the run also
    counts the panels' composition, with ``multiplicity`` (one process, no ``devices``) how often each
    distinct panel was drawn, with ``address`` (what _address_request returned) it is household-aware."""
    from . import distributed as D
    mode = rng or _legacy.RNG_MODE
    if mode not in ("philox", "mt"):
        raise ValueError("rng must be 'philox' or 'mt'")
    enc = encode_cached(instance.categories, instance.agents)
    S = int(iterations)
    ring = _with_address(enc, *address) if address is not None else None
    if mode == "mt":
        import random
        random.seed(random_seed)
        np.random.seed(random_seed)                  # analysis.py:170 (unused by LEGACY)
        enc.check_quotas(instance.k)
        st = np.zeros(3, np.uint64)
        picks, panels, _ = mt_draw(enc, instance.k, S, stats=st, **({} if ring is None else {"addr_next": ring}))
        raw = legacy_sample_device(enc, instance.k, S, random_seed, keep_panels=keep_panels, host_panels=panels,
                                   host_stats=dict(zip(STAT_KEYS, (int(x) for x in st))), groups=groups,
                                   multiplicity=multiplicity)
    elif D.world_size() > 1:
        return LegacyRun(*D.legacy_probabilities_distributed(instance, iterations, random_seed,
                                                             keep_panels=keep_panels, groups=groups))
    else:
        seed(random_seed)
        enc.check_quotas(instance.k)
        STREAM.take_panels(S)
        if devices is not None:
            raw = legacy_sample_raw(enc, instance.k, S, random_seed, want_pairs=True, want_panels=keep_panels,
                                    devices=devices)
        elif ring is not None:
            with _Households(enc, ring):
                raw = legacy_sample_device(enc, instance.k, S, random_seed, keep_panels=keep_panels, groups=groups,
                                           multiplicity=multiplicity)
        else:
            raw = legacy_sample_device(enc, instance.k, S, random_seed, keep_panels=keep_panels, groups=groups,
                                       multiplicity=multiplicity)
    m, dist = raw.multiplicity, None
    if m is not None:
        from .stats import PanelDistribution
        dist = PanelDistribution(S, m["first"], m["mult"], raw.panels, enc.n, enc.agent_ids, spectrum=m["spectrum"],
                                 sum_squares=m["sum_squares"])
    return LegacyRun(*finish(instance, enc, raw, S), composition(groups, raw, S, instance.k), dist)


def composition(groups, raw, S, k):
    """The CompositionHistogram of a run that was given groups (None without)."""
    if groups is None:
        return None
    from .stats import CompositionHistogram
    return CompositionHistogram(groups.labels, raw.composition, S, k)


def legacy_panel_distribution(instance: Instance, iterations: int, random_seed: int, *, rng: str = None,
                              keep_panels: bool = True, columns_data=None, check_same_address_columns=None):
    """``legacy_probabilities`` plus the run as a distribution over whole panels: returns
    ``(alloc, found_panels, pair_histogram, panel_distribution)``.

    The first three are what ``legacy_probabilities(instance, iterations, random_seed, rng=rng,
    keep_panels=keep_panels)`` returns, bit for bit.  ``panel_distribution`` is a
    ``stats.PanelDistribution``: how often each distinct panel was drawn (uq_mult_kernel /
    unique_mult_kernel over the hashes and panels the distinct count already holds, on its side
    stream), the multiplicity spectrum (mult_spectrum_kernel; it rides in the call's one host copy),
    and from them the sample coverage, the Chao1 bound on the panels possible, the collision
    probability and the most frequent panels.  The list stays on the device until read.  The list's
    length must equal ``len(found_panels)`` and the multiplicities must sum to ``iterations``:
    RuntimeError otherwise.  ``rng="mt"`` runs the same passes over the host-drawn panels.  With
    ``keep_panels=False`` the spectrum and estimators work; ``top`` / ``count`` raise.  Sharded runs
    are the sibling's: with torch.distributed initialised and world size > 1 this call raises
    NotImplementedError and ``distributed.legacy_panel_distribution_distributed`` is the call to make (the
    counts travel with the exchange's keys, 32 bytes each).  ``columns_data`` and
    ``check_same_address_columns``: a household-aware run, as ``legacy_probabilities`` takes them."""
    from . import distributed as D
    address = _address_request(instance, columns_data, check_same_address_columns)
    if D.world_size() > 1:
        raise NotImplementedError("legacy_panel_distribution: sharded runs (world size %d) are not supported here; "
                                  "call distributed.legacy_panel_distribution_distributed" % D.world_size())
    run = _legacy_run(instance, iterations, random_seed, keep_panels, rng, None, None, multiplicity=True,
                      address=address)
    return run.alloc, run.panels, run.histogram, run.distribution


def legacy_panel_comparison(instance: Instance, iterations: int, seed_a: int = 0, seed_b: int = 1, *, rng: str = None,
                            columns_data=None, check_same_address_columns=None):
    """Two LEGACY runs of ``iterations`` draws each and their panel tables side by side: returns
    ``(run_a, run_b, comparison)``.

    This is the reference's two-sample design (analyze_instance draws LEGACY with seeds 0 and 1 and reads the
    first sample's minimiser in the second, analysis.py:536-541) carried to whole panels: an estimate made on
    one run is checked on the other.  Each ``run_x`` is what ``legacy_panel_distribution(instance,
    iterations, seed_x, rng=rng)`` returns, bit for bit.  ``comparison`` is the ``stats.PanelComparison`` of the
    two distributions (``stats.compare_panel_distributions``: both runs' kept panels sorted on the device, one
    csa_rows_join_async, 15 words copied): ``mass_b_on_a()`` is the held-out coverage ``run_a``'s Good-Turing
    ``coverage()`` predicts, ``cross_collision()`` the independent estimate beside ``collision_probability()``.
    With torch.distributed initialised and world size > 1 this call raises NotImplementedError, as
    ``legacy_panel_distribution`` does.  ``columns_data`` and ``check_same_address_columns``: both runs
    household-aware, as ``legacy_probabilities`` takes them."""
    from . import distributed as D
    from .stats import compare_panel_distributions
    address = _address_request(instance, columns_data, check_same_address_columns)
    hh = {} if address is None else dict(columns_data=columns_data,
                                         check_same_address_columns=check_same_address_columns)
    if D.world_size() > 1:
        raise NotImplementedError("legacy_panel_comparison: sharded runs (world size %d) are not supported here; "
                                  "call distributed.legacy_panel_distribution_distributed" % D.world_size())
    run_a = legacy_panel_distribution(instance, iterations, seed_a, rng=rng, **hh)
    run_b = legacy_panel_distribution(instance, iterations, seed_b, rng=rng, **hh)
    return run_a, run_b, compare_panel_distributions(run_a[3], run_b[3])


def legacy_initial_committees(instance: Instance, iterations: int, random_seed: int, rounds: int = None, *,
                              rng: str = None, columns_data=None, check_same_address_columns=None):
    """The reference's _generate_initial_committees (xmin.py:229-290) over a LEGACY run's distinct panels instead
    of an ILP: ``legacy_panel_distribution(instance, iterations, random_seed, rng=rng)`` followed by its
    ``initial_committees(rounds)`` (``rounds`` defaults to 3 n, leximin.py:373; csa_rows_mw_cover_async and
    csa_rows_first_holder_async over the run's sorted table on the device).  Returns ``(committees,
    covered_agents, output_lines)``, what _expand_distribution_leximin takes as ``initial_committees`` /
    ``initial_covered_agents``.  World size > 1 raises NotImplementedError, as ``legacy_panel_distribution``;
    ``columns_data`` and ``check_same_address_columns`` are passed on to it."""
    run = legacy_panel_distribution(instance, iterations, random_seed, rng=rng, columns_data=columns_data,
                                    check_same_address_columns=check_same_address_columns)
    return run[3].initial_committees(rounds)


def legacy_maximin(instance: Instance, iterations: int, random_seed: int, rounds: int = None, *, shrink: float = 0.8,
                   resync: int = 16, rng: str = None, columns_data=None, check_same_address_columns=None):
    """How fair could a lottery over exactly the panels a LEGACY run drew be made: ``legacy_panel_distribution(
    instance, iterations, random_seed, rng=rng)`` followed by its ``maximin(rounds, shrink, resync)`` (``rounds``
    defaults to 3 n; csa_rows_maximin_async over the run's sorted table on the device).  Returns a
    ``stats.PanelMaximin``: a ``portfolio()`` that ``portfolio_probabilities``, ``portfolio_composition`` and
    ``legacy_portfolio_overlap`` take, and ``lower <= z* <= upper`` for the optimum z* of the reference's first
    leximin stage over the drawn panels (xmin.py:293-321) -- ``lower`` also bounds LEXIMIN's minimum selection
    probability from below, and the portfolio is a warm start for a caller who has the solvers.  World size > 1
    raises NotImplementedError, as ``legacy_panel_distribution``; ``columns_data`` and
    ``check_same_address_columns`` are passed on to it."""
    run = legacy_panel_distribution(instance, iterations, random_seed, rng=rng, columns_data=columns_data,
                                    check_same_address_columns=check_same_address_columns)
    return run[3].maximin(rounds, shrink, resync)


def legacy_nash(instance: Instance, iterations: int, random_seed: int, rounds: int = 200, *, start: str = "legacy",
                rng: str = None, columns_data=None, check_same_address_columns=None):
    """Which lottery over exactly the panels a LEGACY run drew has the greatest geometric mean of selection
    probabilities, and how much of it does LEGACY leave on the table: ``legacy_panel_distribution(instance,
    iterations, random_seed, rng=rng)`` followed by its ``nash(rounds, start)`` (csa_rows_nash_async over the
    run's sorted table on the device).  Returns a ``stats.PanelNash``: a ``portfolio()`` that
    ``portfolio_probabilities``, ``portfolio_composition`` and ``legacy_portfolio_overlap`` take, and
    ``start_geometric_mean <= geometric_mean <= optimum <= upper`` for the Nash-welfare optimum over the drawn
    panels -- the geometric mean of ``compute_prob_allocation_stats`` (analysis.py:231-255) as an objective.
    ``start="legacy"`` starts from the run's own multiplicities, ``"uniform"`` from equal probabilities.  World
    size > 1 raises NotImplementedError, as ``legacy_panel_distribution``; ``columns_data`` and
    ``check_same_address_columns`` are passed on to it."""
    run = legacy_panel_distribution(instance, iterations, random_seed, rng=rng, columns_data=columns_data,
                                    check_same_address_columns=check_same_address_columns)
    return run[3].nash(rounds, start)


def legacy_price(instance: Instance, weights, iterations: int, random_seed: int, chunk: int = 1 << 20):
    """Heuristic pricing over fresh draws that are not kept: among the panels [0, ``iterations``) of the LEGACY
    stream of ``random_seed``, the one with the largest weight sum.  Returns ``(frozenset of agent ids, value,
    global draw index)``; ties go to the lowest draw index, so the result does not depend on ``chunk``;
    ``(frozenset(), -inf, None)`` for no draws.

    ``weights`` as ``PanelDistribution.price`` takes them (KeyError / ValueError before anything is enqueued).
    Chunks of ``chunk`` panels are drawn on the current device (``distributed.device_redraw``'s
    ``device_chunk``: csa_redraw_async) and each is scored where it lies with csa_rows_price_async(index_base =
    the chunk's offset, CSA_PRICE_ACCUMULATE); one host wait at the end, for the status block and the best pair;
    then the one winning panel is drawn again by its index.  A drawn panel whose value exceeds the LP's bound is a
    violated dual constraint found without an ILP call (xmin.py:410-440).  One process: with world size > 1
    this call raises NotImplementedError."""
    import torch
    from . import distributed as D
    from .stats import PRICE_NONE, RowTable, weight_vector
    if D.world_size() > 1:
        raise NotImplementedError("legacy_price: sharded runs (world size %d) are not supported; price on one "
                                  "process" % D.world_size())
    enc = encode_cached(instance.categories, instance.agents)
    w = weight_vector(weights, enc.agent_ids)
    S, chunk = int(iterations), max(1, int(chunk))
    seed(random_seed)
    enc.check_quotas(instance.k)
    STREAM.take_panels(S)
    dev = torch.device("cuda", torch.cuda.current_device())
    draw = D.device_redraw(enc, instance.k, random_seed, dev)
    ops = draw.tables()
    with torch.cuda.device(dev), torch.cuda.stream(ops.stream):
        d_w = torch.from_numpy(w).to(dev)
        best = torch.tensor([-1, np.array([-np.inf]).view(np.int64)[0]], dtype=torch.int64, device=dev)
        for off in range(0, S, chunk):
            c = min(chunk, S - off)
            length = torch.full((1,), c, dtype=torch.int64, device=dev)
            ops.price(RowTable(draw.device_chunk(off, c), None, None, length, c, enc.W), enc.n, d_w, off, best)
        h = torch.cat([draw.status.view(torch.int64), best]).cpu().numpy()
    N.raise_status(h[:2].view(np.uint32))
    at = int(h[2:3].view(np.uint64)[0])
    if at == PRICE_NONE:
        return frozenset(), float("-inf"), None
    row = np.ascontiguousarray(draw(at, 1), np.uint64).reshape(-1)
    return frozenset(enc.agent_ids[q] for q in unpack_panel(row, enc.n)), float(h[3:4].view(np.float64)[0]), at


def legacy_portfolio_overlap(instance: Instance, distribution, portfolio, probabilities):
    """A LEGACY run's ``stats.PanelDistribution`` beside a LEXIMIN / XMIN ``(portfolio, probabilities)``: how
    much of LEGACY's mass lies on the portfolio's panels and how much of the portfolio's on panels LEGACY ever
    drew -- a ``stats.PortfolioOverlap`` (``stats.portfolio_overlap``: one csa_rows_find_async of the packed
    portfolio in the run's sorted table).  The portfolio is packed as ``portfolio_probabilities`` packs it:
    paired with ``zip``, KeyError for an agent id that is not in the instance."""
    from .stats import portfolio_overlap
    enc = encode_cached(instance.categories, instance.agents)
    pos = getattr(enc, "_pos", None)
    if pos is None:
        pos = enc._pos = {aid: p for p, aid in enumerate(enc.agent_ids)}
    pairs = list(zip(portfolio, probabilities))
    rows = _membership([panel for panel, _ in pairs], enc.n, pos.__getitem__)[1]
    if distribution._n != enc.n or list(distribution._ids or ()) != list(enc.agent_ids):
        raise ValueError("the distribution is over another instance (its agents differ)")
    return portfolio_overlap(distribution, rows, np.array([pob for _, pob in pairs], np.float64).reshape(-1))


def legacy_composition(instance: Instance, iterations: int, random_seed: int, groups, *, rng: str = None,
                       keep_panels: bool = True, columns_data=None, check_same_address_columns=None):
    """``legacy_probabilities`` plus what its panels look like as a whole: returns
    ``(alloc, found_panels, pair_histogram, composition)``.

    The first three are what ``legacy_probabilities(instance, iterations, random_seed, rng=rng,
    keep_panels=keep_panels)`` returns, bit for bit (the same draws: a panel is a pure function of
    seed and panel index).  ``composition`` is a ``stats.CompositionHistogram`` over ``groups`` (a
    ``stats.GroupSet``: ``feature_groups``, ``intersection_groups``, ``agent_groups``, or their sum):
    per group, how many of the run's panels hold 0, 1, ..., k of its members -- group_hist_kernel over
    the drawn panels while they are in device memory, its table returned in the call's one host copy.
    ``rng="mt"`` runs the same pass over the host-drawn panels.  With torch.distributed initialised
    and world size > 1 the call is sharded like ``legacy_probabilities`` and every rank returns the
    whole job's table (summed over the ranks).  ``columns_data`` and ``check_same_address_columns``: a
    household-aware run, as ``legacy_probabilities`` takes them (one rank only); over
    ``stats.household_groups`` its table then holds nothing at two members or more."""
    address = _address_request(instance, columns_data, check_same_address_columns)
    _check_groups(instance, groups)
    return _legacy_run(instance, iterations, random_seed, keep_panels, rng, None, groups, address=address)[:4]


def finish(instance, enc, raw, S):
    global LAST_RUN_STATS
    LAST_RUN_STATS = raw.stats
    # count / S as the reference's int / int true division: both operands are exact in float64 (< 2^53)
    # and IEEE division is correctly rounded, so numpy's float64 quotient is that same value
    alloc = dict(zip(enc.agent_ids, (np.asarray(raw.counts, dtype=np.float64) / float(S)).tolist())) if S else \
        {aid: int(c) / S for aid, c in zip(enc.agent_ids, np.asarray(raw.counts).tolist())}
    hist = PairHistogram(len(instance.agents), counts=raw.pairs)
    hist.turn_into_probabilities_by_dividing_all_elements_by_given_number(S)
    hist._counts, hist._S = raw.pairs, S      # integer counts for stats.sorted_pair_probabilities
    panels = PanelSet(raw.unique, raw.panels, enc.n, enc.agent_ids)
    return alloc, panels, hist


# ---- LEXIMIN / XMIN: everything after the solver (analysis.py:194-228) ----------------------------

def _membership(panels, n, lookup=None):
    """Panels (sized iterables of agent positions 0..n-1, or of keys that ``lookup`` turns into
    positions) -> (x, rows): the P x 64W boolean membership matrix and its uint64[P, W] bitmask rows
    (``xmin.pack_portfolio``'s rows).  One C-level pass over the members; a position outside 0..n-1
    raises KeyError, a panel that names an agent twice ValueError (a bitmask cannot hold it)."""
    from itertools import chain
    W = max((n + 63) // 64, 1)
    panels = [p if hasattr(p, "__len__") else tuple(p) for p in panels]
    P = len(panels)
    lens = np.fromiter(map(len, panels), np.int64, P)
    members = chain.from_iterable(panels)
    flat = np.fromiter(map(lookup, members) if lookup else members, np.int64, int(lens.sum()))
    bad = flat[(flat < 0) | (flat >= n)]
    if bad.size:
        raise KeyError(int(bad[0]))
    x = np.zeros((P, W * 64), np.bool_)
    x[np.repeat(np.arange(P), lens), flat] = True
    if int(np.count_nonzero(x)) != len(flat):
        raise ValueError("a panel of the portfolio names an agent more than once")
    return x, np.ascontiguousarray(np.packbits(x, axis=1, bitorder="little")).view("<u8").reshape(P, W)


def _pack_positions(idx, n):
    """Panels as lists of agent positions (0..n-1) -> uint64[P, W] bitmask rows."""
    return _membership(idx, n)[1]


def _portfolio_launch(rows, weights, n, d_upper, d_alloc, accumulate=False):
    """Upload the packed rows and the weights, transpose (csa_transpose_count_async) and run
    portfolio_pairs_kernel into ``d_upper`` / ``d_alloc`` (device float64 tensors or None), all on the
    outputs' device and its current stream.  Nothing waits for the kernels: the caller reads what it
    needs.  Returns the uploaded ``(rows, weights)`` device tensors (None, None without panels), for a
    caller that runs a second kernel over the same upload."""
    import torch
    L = N.lib()
    P = len(weights) if n else 0
    dev = (d_upper if d_upper is not None else d_alloc).device
    with torch.cuda.device(dev):
        sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        xt = w = d_rows = None
        if P:
            d_rows = torch.from_numpy(rows.view(np.int64).reshape(-1)).to(dev)
            w = torch.from_numpy(np.ascontiguousarray(weights, np.float64)).to(dev)
            xt = torch.empty(((P + 63) // 64) * L.csa_xt_pad(n), dtype=torch.int64, device=dev)
            cnt = torch.zeros(n, dtype=torch.int64, device=dev)     # the transpose's counts: not used
            N.check(L.csa_transpose_count_async(N.ptr(d_rows), P, n, N.ptr(xt), N.ptr(cnt), sp))
        N.check(L.csa_portfolio_pairs_async(N.ptr(xt), P, n, N.ptr(w), N.ptr(d_upper), N.ptr(d_alloc),
                                            N.CSA_PORTFOLIO_ACCUMULATE if accumulate else 0, sp))
    return d_rows, w


def portfolio_probabilities(instance: Instance, portfolio, probabilities, min_probability=None):
    """What the reference's leximin_probabilities / xmin_probabilities compute from the solver's
    ``(portfolio, probabilities)`` (analysis.py:204-210, 222-228), on the device.

    Returns ``(alloc, panels, pair_histogram)``:

    * ``alloc``: ``{agent_id: float}`` over all agents in instance order, each the sum of the
      probabilities of the panels holding the agent, added in portfolio order from ``0.``;
    * ``panels``: the ``set`` of panels as tuples of agent ids -- all of them, or with
      ``min_probability`` those whose probability is ``> min_probability`` (analysis.py:209 uses
      ``1e-11``).  The reference's tuples are in frozenset iteration order; ours are sorted by the
      agents' position in the instance;
    * ``pair_histogram``: every pair's sum of panel probabilities in portfolio order
      (analysis.py:90-95), kept on the device until read.

    Portfolio and probabilities are paired with ``zip`` (the shorter one ends both), as the
    reference does.  An agent id that is not in the instance raises ``KeyError``, as
    ``selection_probs[agent_id] +=`` does there.  Only the packed panels and the weights are
    uploaded; only ``alloc`` and, on first access, the triangle are read back.  Both results are the
    reference's float64 values bit for bit (csa_portfolio_pairs_async's summation-order contract)."""
    return _portfolio_run(instance, portfolio, probabilities, min_probability, None)[:3]


def _portfolio_run(instance, portfolio, probabilities, min_probability, groups):
    """portfolio_probabilities' body; with ``groups`` (a stats.GroupSet) the packed rows and weights it
    uploaded also go through csa_group_whist_async, whose float64[G, k + 1] table and status come back
    in the same host copy as ``alloc``.  Returns (alloc, panels, pair_histogram,
    WeightedCompositionHistogram or None)."""
    import torch
    from .device import StatusBlock
    enc = encode_cached(instance.categories, instance.agents)
    ids, n = enc.agent_ids, enc.n
    pos = getattr(enc, "_pos", None)
    if pos is None:
        pos = enc._pos = {aid: p for p, aid in enumerate(ids)}
    pairs = list(zip(portfolio, probabilities))
    x, rows = _membership([panel for panel, _ in pairs], n, pos.__getitem__)   # KeyError: agent not in the instance
    weights = np.array([pob for _, pob in pairs], np.float64).reshape(-1)
    m = n * (n - 1) // 2
    G, bins = (len(groups), int(instance.k) + 1) if groups is not None else (0, 0)
    tri = torch.empty(max(m, 1), dtype=torch.float64, device="cuda")
    # alloc, then the composition table and its status words: one tensor, one host copy
    out = StatusBlock([("alloc", max(n, 1))] + ([("table", max(G * bins, 1))] if groups is not None else []),
                      torch.float64, "cuda", status=groups is not None)
    d_rows, d_w = _portfolio_launch(rows, weights, n, tri, out.views["alloc"])
    if groups is not None:
        from . import stats as St
        dev = out.out.device
        with torch.cuda.device(dev):
            St.group_whist_device(d_rows, len(weights) if n else 0, enc.W, d_w, groups.device_masks(dev), G, bins,
                                  out.views["table"], out.status, torch.cuda.current_stream(dev))
    # the panel set while the device works: members in ascending position (np.nonzero walks row-major)
    names = list(map(ids.__getitem__, np.nonzero(x)[1].tolist()))
    ends = np.cumsum(np.count_nonzero(x, axis=1)).tolist()
    panels = {tuple(names[a:b]) for a, b, (_, pob) in zip([0] + ends[:-1], ends, pairs)
              if min_probability is None or pob > min_probability}
    total = St.portfolio_total(weights) if groups is not None else None
    h, words = out.host()                                                # the call's one host wait
    alloc = dict(zip(ids, h["alloc"][:n].tolist()))
    comp = None
    if groups is not None:
        N.raise_status(words)
        comp = St.WeightedCompositionHistogram(groups.labels, h["table"][:G * bins].reshape(G, bins).copy(), total,
                                               len(weights), instance.k)
    return alloc, panels, PairHistogram._from_device_triangle(n, tri), comp


def _check_groups(instance, groups):
    """TypeError unless ``groups`` is a stats.GroupSet, ValueError unless it is over the instance's encoding
    -- before a solver runs or anything is uploaded."""
    from .stats import GroupSet
    if not isinstance(groups, GroupSet):
        raise TypeError("groups must be a stats.GroupSet")
    groups.check_width(max((len(instance.agents) + 63) // 64, 1))


def portfolio_composition(instance: Instance, portfolio, probabilities, groups, min_probability=None):
    """``portfolio_probabilities`` plus what the portfolio's panels look like as a whole: returns
    ``(alloc, panels, pair_histogram, composition)``.

    The first three are what ``portfolio_probabilities(instance, portfolio, probabilities,
    min_probability)`` returns, bit for bit.  ``composition`` is a
    ``stats.WeightedCompositionHistogram`` over ``groups`` (a ``stats.GroupSet``: ``feature_groups``,
    ``intersection_groups``, ``agent_groups``, or their sum): per group, the summed probability of the
    panels holding 0, 1, ..., k of its members, each entry added in portfolio order
    (csa_group_whist_async's contract, so ``stats.group_whist_host`` gives the same bits).  It covers
    the whole portfolio whatever ``min_probability`` says, as ``alloc`` does.  The packed rows are
    uploaded once and serve both kernels; the table comes back in the call's one host wait.
    ``stats.composition_difference`` sets it against ``legacy_composition``'s.  ``groups`` that is
    not a GroupSet raises TypeError, one of another encoding ValueError."""
    _check_groups(instance, groups)
    return _portfolio_run(instance, portfolio, probabilities, min_probability, groups)


def _solver(module, name):
    """The reference's solver entry point if its module is importable; else ImportError naming the
    ``find_distribution`` keyword."""
    import importlib
    try:
        fn = getattr(importlib.import_module(module), name, None)
    except ImportError:
        fn = None
    if fn is None:
        raise ImportError("%s.%s is not importable (the solver stays in the reference and needs Gurobi): pass the "
                          "solver as find_distribution=, called as find_distribution(categories, agents, "
                          "columns_data, k, False, [])" % (module, name))
    return fn


def _solved_probabilities(instance, find_distribution, min_probability, groups=None):
    columns_data = {agent_id: {} for agent_id in instance.agents}
    portfolio, output_probs, _ = find_distribution(instance.categories, instance.agents, columns_data, instance.k,
                                                   False, [])
    if groups is not None:
        return portfolio_composition(instance, portfolio, output_probs, groups, min_probability=min_probability)
    return portfolio_probabilities(instance, portfolio, output_probs, min_probability=min_probability)


def leximin_probabilities(instance: Instance, find_distribution=None) -> Tuple[ProbAllocation, set, PairHistogram]:
    """analysis.py:194-210: the exact probability allocation for LEXIMIN.  ``find_distribution`` is the
    solver (default: the reference's ``leximin.find_distribution_leximin`` when importable, else
    ImportError), called as the reference calls it; the rest is ``portfolio_probabilities`` with
    the reference's ``1e-11`` threshold on the returned set of panels."""
    if find_distribution is None:
        find_distribution = _solver("leximin", "find_distribution_leximin")
    return _solved_probabilities(instance, find_distribution, 0.00000000001)


def xmin_probabilities(instance: Instance, find_distribution=None) -> Tuple[ProbAllocation, set, PairHistogram]:
    """analysis.py:213-228: the same for XMIN (default solver: the reference's
    ``xmin.find_distribution_xmin``); every panel of the portfolio is in the returned set."""
    if find_distribution is None:
        find_distribution = _solver("xmin", "find_distribution_xmin")
    return _solved_probabilities(instance, find_distribution, None)


def leximin_composition(instance: Instance, groups, find_distribution=None):
    """``leximin_probabilities`` plus the weighted composition of the LEXIMIN portfolio over ``groups``:
    ``(alloc, panels, pair_histogram, composition)`` (see ``portfolio_composition``).  The solver is passed
    or found as there.  The ``1e-11`` threshold applies to the returned panel set only: the composition
    covers the whole portfolio, as the marginals do."""
    _check_groups(instance, groups)
    if find_distribution is None:
        find_distribution = _solver("leximin", "find_distribution_leximin")
    return _solved_probabilities(instance, find_distribution, 0.00000000001, groups)


def xmin_composition(instance: Instance, groups, find_distribution=None):
    """The same for XMIN (default solver: the reference's ``xmin.find_distribution_xmin``)."""
    _check_groups(instance, groups)
    if find_distribution is None:
        find_distribution = _solver("xmin", "find_distribution_xmin")
    return _solved_probabilities(instance, find_distribution, None, groups)
