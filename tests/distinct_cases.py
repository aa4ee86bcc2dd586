"""Forged inputs for the distinct-panel kernels (csrc/csa_legacy.hip: unique_kernel and the uq_* pass).

Pure numpy.  Every builder returns a `Case`, a 3-tuple `(hashes uint64[n, 2], panels uint64[n, W],
expected)` whose `expected` distinct count is known BY CONSTRUCTION: the builder makes D distinct
triples (h1, h2, row), appends n - D copies of them, and applies a fixed permutation so that copies of
one triple land in different CH chunks and different waves -- so expected = D, whatever the code under
test says.  The kernels' stated rule is the reference semantics: two entries are the same panel iff
h1, h2 AND the row are all equal.  `Case.distinct_hashes` / `Case.distinct_panels` hold the D triples
for the exchange checks.

The hard cases never occur with honest hashes of honest draws, so the hashes are forged; the small
mirrors of the routing arithmetic below (`part`, `lds_slot`, `global_slot`, `plan`) aim them.
tests/test_distinct_cases_host.py pins what the builders produce on the CPU; tests/test_gpu_distinct.py
runs them through the C ABI.
"""
import numpy as np

from conftest import pkg

K_UQ_TABLE = 8192       # kUqTable: LDS slots of one partition's table
K_UQ_MAX_PARTS = 8192   # kUqMaxParts
K_UQ_THREADS = 256      # kUqThreads (uq_scan_part_kernel); uq_scan_tot_kernel runs 1024 threads
PART_MIN = 65536        # unique_impl: smaller calls take the single global table
ONE_PART_TOP13 = 0x16ED  # the partition of one_partition_* (top 13 bits of h1)
SEG_CAP = 9973
SEG_COUNTS = (SEG_CAP, 0, 1, SEG_CAP - 1, 5000, SEG_CAP, 17, 0)

_U = np.uint64


# ---- mirrors of the routing arithmetic ----------------------------------------------------------
def part(h1, pbits):
    """uq_part: the partition of a hash is the top pbits bits of h1."""
    return np.asarray(h1, _U) >> _U(64 - pbits)


def lds_slot(h1, h2):
    """uq_dedupe_kernel: the first probed slot of the partition's LDS table."""
    return (np.asarray(h1, _U) ^ (np.asarray(h2, _U) >> _U(29))) & _U(K_UQ_TABLE - 1)


def global_slot(h1, h2, slots):
    """unique_kernel: the first probed slot of a global table of `slots` (a power of two) slots."""
    return (np.asarray(h1, _U) ^ (np.asarray(h2, _U) >> _U(29))) & _U(slots - 1)


def plan(n):
    """uq_plan restated: (pbits, P, CH, nwg) of a partitioned pass over n entries."""
    pbits = 6
    while (1 << pbits) * 1024 < n and pbits < 13:
        pbits += 1
    CH = max(4096, ((n + 1023) // 1024 + 255) // 256 * 256)
    return pbits, 1 << pbits, CH, (n + CH - 1) // CH


def scan_per(n):
    """Elements per thread of (uq_scan_part_kernel, uq_scan_tot_kernel) for n entries."""
    _, P, _, nwg = plan(n)
    return (nwg + K_UQ_THREADS - 1) // K_UQ_THREADS, (P + 1023) // 1024


def table_slots(n):
    """Slots of the table a caller brings for n entries (distributed.HashTable): pow2 >= 2 n, >= 64."""
    slots = 64
    while slots < 2 * max(int(n), 1):
        slots <<= 1
    return slots


def scratch_bytes(n):
    """UqPlan::scratch_bytes: idx[n] | hist[P nwg] | tot[P] | base[P + 1], all uint32."""
    _, P, _, nwg = plan(n)
    return 4 * n + 4 * P * nwg + 4 * P + 4 * (P + 1)


def fits(n):
    """UqPlan::fits."""
    return n < (1 << 31) and n // plan(n)[1] <= 2048


def takes_partitioned(n, slots):
    """unique_impl's choice with a status block and CSA_UNIQUE_PART unset."""
    return n >= PART_MIN and fits(n) and scratch_bytes(n) <= 8 * slots


# ---- building blocks ---------------------------------------------------------------------------
class Case(tuple):
    """(hashes, panels, expected) plus the D distinct triples the entries were copied from."""

    def __new__(cls, hashes, panels, distinct_hashes, distinct_panels):
        self = super().__new__(cls, (hashes, panels, len(distinct_hashes)))
        self.distinct_hashes = distinct_hashes
        self.distinct_panels = distinct_panels
        return self


def honest_hashes(rows):
    return pkg("distributed").panel_hashes(rows)


def _rows(rng, D, W):
    """D random rows, pairwise different."""
    r = rng.integers(0, 2 ** 64, size=(D, W), dtype=np.uint64)
    assert len(np.unique(r, axis=0)) == D
    return r


def set_top(h1, value, bits):
    """h1 with its top `bits` bits replaced by `value`."""
    low = _U((1 << (64 - bits)) - 1)
    return (np.asarray(h1, _U) & low) | (np.asarray(value, _U) << _U(64 - bits))


def _assemble(dh, dp, n, rng, copies=None):
    """Each of the D triples once, then the copies (indices into the triples; default: n - D drawn
    at random), then the fixed permutation."""
    D = len(dh)
    assert len(dp) == D and D <= n
    assert len(np.unique(dp, axis=0)) == D       # different rows: the triples differ whatever the hashes
    if copies is None:
        copies = rng.integers(0, D, size=n - D)
    idx = np.concatenate([np.arange(D), np.asarray(copies, np.int64)])
    assert len(idx) == n
    idx = idx[rng.permutation(n)]
    return Case(np.ascontiguousarray(dh[idx]), np.ascontiguousarray(dp[idx]), dh, dp)


# ---- builders ----------------------------------------------------------------------------------
def honest(n, W, seed):
    """Honest hashes of random rows; 3/4 of the entries are duplicates."""
    rng = np.random.default_rng(seed)
    dp = _rows(rng, n // 4, W)
    return _assemble(honest_hashes(dp), dp, n, rng)


def honest_large(n=1050001):
    return honest(n, 1, 101)


def threshold(n):
    return honest(n, 2, 107)


def skewed_large(n=1050001):
    """About 30 % of the entries forced into 5 partitions (the first, the last and three inside) by the
    top bits of h1: each holds 6 % of the entries and at most 4000 distinct triples; the rest is honest."""
    rng = np.random.default_rng(103)
    pbits, P, _, _ = plan(n)
    forced = [0, 1, P // 2 - 1, P // 2, P - 1]
    per = int(0.06 * n)
    d_forced = min(4000, per // 15)
    n_honest = n - len(forced) * per
    d_honest = n_honest // 4
    dp = _rows(rng, len(forced) * d_forced + d_honest, 1)
    dh = honest_hashes(dp)
    copies = []
    for j, f in enumerate(forced):
        a = j * d_forced
        dh[a:a + d_forced, 0] = set_top(dh[a:a + d_forced, 0], f, pbits)
        copies.append(a + rng.integers(0, d_forced, size=per - d_forced))
    a = len(forced) * d_forced
    copies.append(a + rng.integers(0, d_honest, size=n_honest - d_honest))
    return _assemble(dh, dp, n, rng, np.concatenate(copies))


def one_partition(D, n, seed=109):
    """D distinct triples whose h1 all share their top 13 bits (one partition at every pbits), the low
    bits honest; n - D duplicates.  The first 8192 triples are the same for every D >= 8192."""
    rng = np.random.default_rng(seed)
    assert D <= K_UQ_TABLE + 64
    dp = _rows(rng, K_UQ_TABLE + 64, 3)[:D]
    dh = honest_hashes(dp)
    dh[:, 0] = set_top(dh[:, 0], ONE_PART_TOP13, 13)
    return _assemble(dh, dp, n, np.random.default_rng(seed + 1))


def one_partition_full():
    return one_partition(K_UQ_TABLE, 70000)


def one_partition_over():
    return one_partition(K_UQ_TABLE + 1, 70001)


def collision_chains(n=66000, groups=2000, members=5, W=3):
    """`groups` groups of `members` different rows under ONE (h1, h2) each (the honest hash of the
    group's first row); the rows of a group differ only in word W - 1.  Every triple occurs at least
    twice."""
    rng = np.random.default_rng(113)
    base = _rows(rng, groups, W)
    dp = np.repeat(base, members, axis=0)
    dp[:, W - 1] += np.tile(np.arange(members, dtype=np.uint64), groups)     # wraps mod 2^64
    dh = np.repeat(honest_hashes(base), members, axis=0)
    D = groups * members
    assert np.array_equal(dp[:, : W - 1], np.repeat(base[:, : W - 1], members, axis=0))
    copies = np.concatenate([np.arange(D), rng.integers(0, D, size=n - 2 * D)])
    return _assemble(dh, dp, n, rng, copies)


PILEUP = 300


def slot_pileup(n=66000, slots=None):
    """PILEUP distinct triples with pairwise different hashes in one partition, whose first LDS slot is
    8190 or 8191 (the chain wraps to slot 0) and whose first slot in a global table of `slots` slots
    (default: table_slots(n)) is slots - 2 or slots - 1 (that chain wraps too); each occurs at least
    twice.  They come first among the distinct triples; the remainder is honest."""
    slots = slots or table_slots(n)
    assert slots >= K_UQ_TABLE and slots & (slots - 1) == 0 and slots <= 1 << 51
    rng = np.random.default_rng(127)
    d_honest = (n - 2 * PILEUP) // 4
    dp = _rows(rng, PILEUP + d_honest, 2)
    dh = honest_hashes(dp)
    h2 = rng.integers(0, 2 ** 64, size=PILEUP, dtype=np.uint64)
    target = _U(slots - 1) - (np.arange(PILEUP, dtype=np.uint64) & _U(1))
    h1 = set_top(rng.integers(0, 2 ** 64, size=PILEUP, dtype=np.uint64), ONE_PART_TOP13, 13)
    h1 = (h1 & ~_U(slots - 1)) | (target ^ ((h2 >> _U(29)) & _U(slots - 1)))
    dh[:PILEUP, 0] = h1
    dh[:PILEUP, 1] = h2
    assert len(np.unique(dh[:PILEUP], axis=0)) == PILEUP
    D = len(dh)
    copies = np.concatenate([np.arange(PILEUP), rng.integers(0, D, size=n - D - PILEUP)])
    return _assemble(dh, dp, n, rng, copies)


def full_pileup(n=66000):
    """The longest probe the LDS table allows: 8192 distinct triples with pairwise different hashes in
    one partition, ALL with first LDS slot 8191, each exactly twice.  Whichever of them a workgroup
    inserts last finds the one free slot only at its 8192nd probe (the slot just before its first), and
    that triple's copy finds its match there.  one_partition_full fills the table too, but with honest
    low bits, where a probe of that length does not occur.  The remainder is honest and kept out of
    that partition."""
    rng = np.random.default_rng(139)
    pbits = plan(n)[0]
    d_honest = (n - 2 * K_UQ_TABLE) // 4
    dp = _rows(rng, K_UQ_TABLE + d_honest, 2)
    dh = honest_hashes(dp)
    h2 = dh[:K_UQ_TABLE, 1]
    h1 = set_top(dh[:K_UQ_TABLE, 0], ONE_PART_TOP13, 13)
    top = _U(K_UQ_TABLE - 1)
    dh[:K_UQ_TABLE, 0] = (h1 & ~top) | (top ^ ((h2 >> _U(29)) & top))
    assert len(np.unique(dh[:K_UQ_TABLE], axis=0)) == K_UQ_TABLE
    hh = dh[K_UQ_TABLE:, 0]
    hh[part(hh, pbits) == _U(ONE_PART_TOP13 >> (13 - pbits))] ^= _U(1 << 63)
    copies = np.concatenate([np.arange(K_UQ_TABLE),
                             K_UQ_TABLE + rng.integers(0, d_honest, size=n - 2 * K_UQ_TABLE - d_honest)])
    return _assemble(dh, dp, n, rng, copies)


# ---- segmented layout (the owner side of the exchange) -----------------------------------------
def segments(case, cap=SEG_CAP, counts=SEG_COUNTS, seed=131):
    """Lay a case's entries out as len(counts) segments of `cap` slots, the first counts[s] slots of
    segment s valid (sum(counts) == the case's n), every other slot poisoned: half the poison are
    triples found nowhere else -- fresh rows, every other one under the hash of a valid triple --
    which would inflate the count if read, half are copies of valid triples.
    Returns (hashes uint64[S * cap, 2], panels uint64[S * cap, W], counts uint64[S], expected)."""
    h, p, expected = case
    n, W = p.shape
    counts = np.asarray(counts, np.int64)
    assert counts.sum() == n and (counts <= cap).all()
    total = len(counts) * cap
    rng = np.random.default_rng(seed)
    n_bad = total - n
    n_fresh = n_bad // 2
    fresh_p = _rows(rng, n_fresh, W)
    assert len(np.unique(np.concatenate([case.distinct_panels, fresh_p]), axis=0)) == expected + n_fresh
    fresh_h = honest_hashes(fresh_p)
    fresh_h[::2] = h[rng.integers(0, n, size=len(fresh_h[::2]))]
    pick = rng.integers(0, n, size=n_bad - n_fresh)
    bad_h = np.concatenate([fresh_h, h[pick]])
    bad_p = np.concatenate([fresh_p, p[pick]])
    order = rng.permutation(n_bad)
    bad_h, bad_p = bad_h[order], bad_p[order]
    slot = np.arange(total)
    valid = (slot % cap) < counts[slot // cap]
    oh = np.empty((total, 2), np.uint64)
    op = np.empty((total, W), np.uint64)
    oh[valid], op[valid] = h, p
    oh[~valid], op[~valid] = bad_h, bad_p
    return oh, op, counts.astype(np.uint64), expected


def segment_source(kind):
    """The two cases the segmented tests lay out: sum(SEG_COUNTS) entries each."""
    n = int(sum(SEG_COUNTS))
    return honest(n, 2, 137) if kind == "honest" else collision_chains(n)


# every csa_unique_async case by name (the GPU test's parametrisation; the host test pins the small ones)
UNIQUE_CASES = {
    "honest_large_1050001": lambda: honest_large(1050001),
    "honest_large_4200001": lambda: honest_large(4200001),
    "skewed_large": skewed_large,
    "one_partition_full": one_partition_full,
    "one_partition_over": one_partition_over,
    "collision_chains": collision_chains,
    "slot_pileup": slot_pileup,
    "full_pileup": full_pileup,
    "threshold_65535": lambda: threshold(65535),
    "threshold_65536": lambda: threshold(65536),
    "threshold_65537": lambda: threshold(65537),
}
