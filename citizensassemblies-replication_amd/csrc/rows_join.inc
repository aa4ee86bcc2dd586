// rows_join.inc -- two sorted distinct-row tables side by side: the join of A and B (which rows are in A
// only, in B only, in both, with both multiplicities and an exact integer summary of the whole union) and
// the lookup of a few rows in one table.  Included by csa_legacy.hip inside an anonymous namespace, after
// distinct_rows.inc, whose records, merge pass and scan it reuses as they are (kernels are templates of an
// unused parameter for the reason given in multiplicity_exchange.inc's "Layout": every kernel that existed
// keeps its offset in the code object).
//
// The join is the merge's first two passes (rs_records_kernel, one rs_merge_kernel pass over the single pair
// of runs) and then its own compaction.  After the merge pass a run of equal rows has length 1 or 2, since
// each table is distinct; rs_less breaks ties by record index and A's records lie below `split`, so in a run
// of two the head is A's record and its successor is B's.
//
//   rj_flag_kernel     cls[i] = the class of the union row that record i heads (1: only in A, 2: only in
//                      B, 4: in both; 0: record i is the second of its run), the selected heads per block,
//                      and the block's share of the summary as kRjWords integers in a slab;
//   rs_scan_kernel     (distinct_rows.inc) exclusive scan of the block counts, *d_out_len, the overflow
//                      check against cap_out;
//   rj_summary_kernel  one workgroup adds the slab's rows into the record and checks the 64-bit fit;
//   rj_pos_kernel      pos[o] = position of the o-th selected head (rs_pos_kernel reads a flag byte as a
//                      count, a class byte is none);
//   rj_gather_kernel   out row o = the row of record pos[o]; mult_a / mult_b from the head and, in class
//                      4, its successor.
//
// Sums.  Every value is an unsigned integer sum, so any order of addition gives the same words: wave
// shuffles, then LDS, then the slab, then one workgroup.  Words 0..7 cannot leave 64 bits (fewer than 2^32
// rows of 32-bit multiplicities); words 8 and 9 add products below 2^64 and are carried as (low, high)
// pairs up to the summary kernel, which reports a non-zero high word in word 10.  No float anywhere.
//
// Trip counts.  As distinct_rows.inc: the binary searches by 33 halvings, row compares by W, the slab walk
// by the block count of the host capacity; lengths read from the device are clamped to the host capacities
// before use.
constexpr int kRjWords = 12;   // slab row: record words 0..7, then (low, high) of words 8 and 9
constexpr uint32_t kRjOnlyA = 1, kRjOnlyB = 2, kRjBoth = 4;
constexpr uint32_t kRjMissing = 0xFFFFFFFFu;

struct RjMult {   // NULL: every multiplicity of that table is 1
    const uint32_t *a, *b;
    uint64_t scale_a, scale_b;
};

__device__ __forceinline__ void rj_add128(uint64_t *lohi, uint64_t x) {
    const uint64_t lo = lohi[0] + x;
    lohi[1] += lo < x ? 1u : 0u;
    lohi[0] = lo;
}

// v[0..7] plain 64-bit sums, (v[8], v[9]) and (v[10], v[11]) 128-bit sums
__device__ __forceinline__ void rj_add(uint64_t *v, const uint64_t *o) {
    for (int w = 0; w < 8; ++w) v[w] += o[w];
    for (int w = 8; w < kRjWords; w += 2) {
        rj_add128(v + w, o[w]);
        v[w + 1] += o[w + 1];
    }
}

// the workgroup's sum of v into thread 0's v (s_part: kRsThreads / 64 rows of kRjWords words)
__device__ __forceinline__ void rj_block_sum(uint64_t *v, uint64_t *s_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d > 0; d >>= 1) {
        uint64_t o[kRjWords];
        for (int w = 0; w < kRjWords; ++w) o[w] = (uint64_t)__shfl_down((unsigned long long)v[w], d);
        if (lane + d < 64) rj_add(v, o);
    }
    if (lane == 0)
        for (int w = 0; w < kRjWords; ++w) s_part[wave * kRjWords + w] = v[w];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < kRsThreads / 64; ++q) rj_add(v, s_part + q * kRjWords);
}

// cls, the selected heads per block, the block's slab row (grid over the host capacity: blocks past the
// length write a zero count and a zero row)
template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rj_flag_kernel(RsSrc src, RsLen len, RjMult mu, uint32_t select,
                                                             const uint64_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ idx,
                                                             uint8_t *__restrict__ cls, uint32_t *__restrict__ bc,
                                                             uint64_t *__restrict__ slab) {
    __shared__ uint32_t s_wave[kRsThreads / 64];
    __shared__ uint64_t s_part[(kRsThreads / 64) * kRjWords];
    const uint64_t n = len.total();
    uint32_t c = 0;
    uint64_t v[kRjWords];
    for (int w = 0; w < kRjWords; ++w) v[w] = 0;
    for (int q = 0; q < kRsPer; ++q) {
        const uint64_t i = (uint64_t)blockIdx.x * kRsTile + q * kRsThreads + threadIdx.x;
        if (i >= n) continue;
        const uint64_t k = keys[i];
        const uint32_t r = idx[i];
        uint32_t what = 0;
        if (i == 0 || !rs_same_row(src, keys[i - 1], idx[i - 1], k, r)) {
            const bool in_a = r < src.split;
            uint32_t r2 = 0;
            bool both = false;
            if (in_a && i + 1 < n) {
                r2 = idx[i + 1];
                both = r2 >= src.split && rs_same_row(src, k, r, keys[i + 1], r2);
            }
            what = both ? kRjBoth : in_a ? kRjOnlyA : kRjOnlyB;
            const uint64_t ma = in_a ? (mu.a ? mu.a[r] : 1u) : 0u;
            const uint64_t mb = both ? (mu.b ? mu.b[r2 - src.split] : 1u)
                                     : in_a ? 0u : (mu.b ? mu.b[r - src.split] : 1u);
            v[0] += 1;
            v[1] += both ? 1u : 0u;
            v[2] += what == kRjOnlyA ? 1u : 0u;
            v[3] += what == kRjOnlyB ? 1u : 0u;
            v[4] += ma;
            v[5] += mb;
            if (both) {
                v[6] += ma;
                v[7] += mb;
                rj_add128(v + 8, ma * mb);   // every factor is below 2^32
                rj_add128(v + 10, min(ma * mu.scale_b, mb * mu.scale_a));
            }
        }
        cls[i] = (uint8_t)what;
        c += (what & select) ? 1u : 0u;
    }
    uint32_t total;
    rs_block_scan(c, s_wave, &total);
    rj_block_sum(v, s_part);
    if (threadIdx.x == 0) {
        bc[blockIdx.x] = total;
        for (int w = 0; w < kRjWords; ++w) slab[(uint64_t)blockIdx.x * kRjWords + w] = v[w];
    }
}

// one workgroup: record[0..10] from the n_blocks slab rows
template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rj_summary_kernel(const uint64_t *__restrict__ slab, uint64_t n_blocks,
                                                                unsigned long long *__restrict__ record,
                                                                uint32_t *__restrict__ status) {
    __shared__ uint64_t s_part[(kRsThreads / 64) * kRjWords];
    uint64_t v[kRjWords];
    for (int w = 0; w < kRjWords; ++w) v[w] = 0;
    for (uint64_t b = threadIdx.x; b < n_blocks; b += kRsThreads) rj_add(v, slab + b * kRjWords);
    rj_block_sum(v, s_part);
    if (threadIdx.x == 0) {
        for (int w = 0; w < 8; ++w) record[w] = v[w];
        record[8] = v[8];
        record[9] = v[10];
        const bool over = (v[9] | v[11]) != 0;
        record[10] = over ? 1u : 0u;
        if (over) raise_status(status, CSA_E_UNSUPPORTED, 0xFFFFFFFFFFFFFFFFull);
    }
}

template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rj_pos_kernel(RsLen len, uint32_t select, const uint8_t *__restrict__ cls,
                                                            const uint32_t *__restrict__ bc, uint32_t *__restrict__ pos) {
    __shared__ uint32_t s_wave[kRsThreads / 64];
    const uint64_t n = len.total();
    const uint64_t i0 = (uint64_t)blockIdx.x * kRsTile + (uint64_t)threadIdx.x * kRsPer;
    uint32_t f[kRsPer], c = 0;
    for (int q = 0; q < kRsPer; ++q) {
        f[q] = i0 + q < n && (cls[i0 + q] & select) ? 1u : 0u;
        c += f[q];
    }
    uint32_t total;
    uint32_t o = bc[blockIdx.x] + rs_block_scan(c, s_wave, &total);
    for (int q = 0; q < kRsPer; ++q)
        if (f[q]) pos[o++] = (uint32_t)(i0 + q);   // o < the selected count <= n: pos holds n + 1 words
}

// out row o (o < min(selected count, cap_out)) = the row of record pos[o]; grid-stride over the rows' words
template <int kLate = 0>
__global__ void rj_gather_kernel(RsSrc src, RjMult mu, const uint32_t *__restrict__ idx, const uint8_t *__restrict__ cls,
                                 const uint32_t *__restrict__ pos, const unsigned long long *__restrict__ out_len,
                                 uint64_t cap_out, uint64_t *__restrict__ out_rows, uint32_t *__restrict__ out_mult_a,
                                 uint32_t *__restrict__ out_mult_b) {
    const uint64_t D = min((uint64_t)*out_len, cap_out), words = D * src.W;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += step) {
        const uint64_t o = t / src.W;
        const int w = (int)(t - o * src.W);
        const uint32_t p = pos[o], r = idx[p];
        if (out_rows) out_rows[t] = src.row(r)[w];
        if (w) continue;
        const uint32_t what = cls[p];
        const bool in_a = r < src.split;
        const uint32_t rb = what == kRjBoth ? idx[p + 1] : r;   // class 4: record p + 1 exists and is B's
        if (out_mult_a) out_mult_a[o] = in_a ? (mu.a ? mu.a[r] : 1u) : 0u;
        if (out_mult_b) out_mult_b[o] = (what == kRjBoth || !in_a) ? (mu.b ? mu.b[rb - src.split] : 1u) : 0u;
    }
}

// out[q] = the index of the table row equal to query q, or kRjMissing (one thread per query)
template <int kLate = 0>
__global__ void rj_find_kernel(const uint64_t *__restrict__ rows, const unsigned long long *__restrict__ d_len,
                               uint64_t cap, int W, const uint64_t *__restrict__ queries, uint64_t n_queries,
                               uint32_t *__restrict__ out) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries) return;
    const uint64_t *want = queries + q * W;
    uint64_t lo = 0, hi = min((uint64_t)*d_len, cap);   // cap < 2^32 - 1: 33 halvings empty any range
    const uint64_t n = hi;
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t *row = rows + mid * W;
        bool below = false;   // row < want
        for (int w = 0; w < W; ++w) {
            const uint64_t a = row[w], b = want[w];
            if (a != b) {
                below = a < b;
                break;
            }
        }
        if (below) lo = mid + 1;
        else hi = mid;
    }
    uint32_t at = kRjMissing;
    if (lo < n) {
        const uint64_t *row = rows + lo * W;
        bool same = true;
        for (int w = 0; w < W; ++w) same = same && row[w] == want[w];
        if (same) at = (uint32_t)lo;
    }
    out[q] = at;
}

struct RjLayout {
    RsLayout rs;
    uint64_t slab, bytes;
};

__host__ inline RjLayout rj_layout(uint64_t n_records) {
    RjLayout J;
    J.rs = rs_layout(n_records);
    J.slab = J.rs.bytes;                                    // u64[n_blocks][kRjWords]
    J.bytes = J.slab + 8 * kRjWords * J.rs.n_blocks;
    return J;
}
