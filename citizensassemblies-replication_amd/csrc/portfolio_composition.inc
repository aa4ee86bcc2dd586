// portfolio_composition.inc -- whist_count_kernel + whist_sum_kernel: the weighted group composition of a
// LEXIMIN / XMIN portfolio.  Included by csa_legacy.hip inside its anonymous namespace.
//
// group_hist_kernel (composition.inc) counts the panels of a LEGACY run per (group, members held).  A
// portfolio's panels carry float64 probabilities, so its composition is a float64 sum per entry, and
// float64 addition does not associate: like portfolio_pairs_kernel (portfolio.inc) this pair of kernels
// fixes the summation order, so that a host loop is the yardstick bit for bit.
//
// Contract, per group g and c in [0, bins): hist[g][c] starts from +0.0 (or from the stored value when
// accumulating) and receives w[p] for every panel p with popcount(panel_p & mask_g) == c, in ASCENDING
// p, one plain IEEE float64 add each.  One thread owns a group's whole row for the whole panel range:
// no tree reduction, no split of an entry's panels over threads, no atomics on the values, no multiply
// (nothing to contract into an FMA); the build has no -ffast-math (see _native.build).
//
// Shape: two passes.  The counts are integers and order-free, the sums are ordered and cheap:
//
//   whist_count_kernel   group_hist_kernel's loop (lane = group, a slab's masks word-major in LDS, the
//                        panel words at a wave-uniform address, two panels per pass, panels over waves
//                        and workgroups) with a store where the atomic was: counts[p][g] as u32, 256
//                        contiguous bytes per wave.  A count >= bins raises CSA_E_INVALID with the panel
//                        index here, where every panel has a wave of its own.
//   whist_sum_kernel     one wave per slab of up to 64 groups, lane = group.  It walks the panels in
//                        ascending p: the weights of kWhChunk panels are staged in LDS, and the lane's
//                        counts (coalesced rows of counts[p]) are fetched kWhUnroll at a time into one
//                        of two register sets, one block ahead of their adds, so that the loads'
//                        latency lies under the previous block.  Each count then takes its weight into
//                        the lane's own float64 row: kWhBlock panels' entries are read together, added
//                        to in ascending p with the sum forwarded in registers where two panels of the
//                        block hit one entry, and stored in order.  The rows sit in LDS ([slab] rows of
//                        bins + 1 entries, padded to an odd length so that the lanes of a wave fall on
//                        different banks unless their counts differ as their rows do), loaded from
//                        d_hist or zeroed at the start and stored whole at the end -- every entry is
//                        written.  The spare entry takes the adds that must not count (a count no bin
//                        has, a lane without a group), so the loop has no predication.  One wave
//                        issues every instruction of a slab's P panels, so the pass is bound by
//                        instructions per panel, whatever the number of lanes; where 64 rows exceed
//                        the LDS the slab is halved until they fit (64 groups to 302 bins, 32 to 606,
//                        ... one group to 19 454): more workgroups, not more time.  Past that the row
//                        is d_hist itself (zeroed by the enqueue unless accumulating, stores
//                        predicated): the same adds in the same order, so the same bits, at a global
//                        round trip per block.
//
// Entries no panel reaches are never added to: they keep +0.0 or, accumulating, their stored bits (the
// rows move as 64-bit words, so a -0.0 or a NaN payload survives).  Every d_hist index is g * bins + c
// with g < n_groups and c < bins checked at the store.
constexpr int kWhThreads = 1024;  // whist_count_kernel: sixteen waves share a slab's masks
constexpr int kWhWaves = kWhThreads / 64;
constexpr int kWhTargetBlocks = 1024;  // count pass: four workgroups per CU's worth of panel ranges
constexpr int kWhSlab = 64;            // whist_sum_kernel: one wave; up to this many groups (lanes) per workgroup
constexpr int kWhChunk = 1024;         // whist_sum_kernel: weights staged in LDS per barrier pair (8 KB)
constexpr int kWhUnroll = 32;          // whist_sum_kernel: counts fetched this many panels ahead of their adds
constexpr int kWhBlock = 4;            // whist_sum_kernel: panels whose entries are read together
static_assert(kWhChunk % kWhUnroll == 0 && kWhChunk % kWhSlab == 0 && kWhUnroll % kWhBlock == 0, "whole blocks");

__global__ __launch_bounds__(kWhThreads) void whist_count_kernel(const uint64_t *__restrict__ panels,
                                                                 uint64_t n_panels, int W,
                                                                 const uint64_t *__restrict__ masks, int n_groups,
                                                                 int bins, int slab,
                                                                 uint32_t *__restrict__ counts,
                                                                 uint32_t *__restrict__ status) {
    extern __shared__ uint64_t smem[];
    uint64_t *s_mask = smem;  // [W][slab]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g0 = (int)blockIdx.x * slab;
    const int ng = min(slab, n_groups - g0);

    for (int e = t; e < W * slab; e += kWhThreads) {  // global reads run along a mask's words
        const int j = e / W, w = e - j * W;
        s_mask[w * slab + j] = j < ng ? masks[(size_t)(g0 + j) * W + w] : 0ull;
    }
    __syncthreads();

    const bool active = lane < ng;
    const int li = active ? lane : 0;  // idle lanes read a valid word and store nothing
    const uint64_t *mrow = s_mask + li;
    uint32_t *crow = counts + (g0 + li);
    const uint64_t step = (uint64_t)gridDim.y * kWhWaves;
    for (uint64_t p0 = (uint64_t)blockIdx.y * kWhWaves + wave; p0 < n_panels; p0 += 2 * step) {
        const uint64_t p1 = p0 + step;
        const bool two = p1 < n_panels;  // wave-uniform
        const uint64_t *a = panels + p0 * (uint64_t)W;
        const uint64_t *b = two ? panels + p1 * (uint64_t)W : a;
        int c0 = 0, c1 = 0;
        for (int w = 0; w < W; ++w) {
            const uint64_t m = mrow[w * slab];
            c0 += __popcll(a[w] & m);
            c1 += __popcll(b[w] & m);
        }
        if (active) {
            crow[p0 * (uint64_t)n_groups] = (uint32_t)c0;
            if (c0 >= bins) raise_status(status, CSA_E_INVALID, p0);
            if (two) {
                crow[p1 * (uint64_t)n_groups] = (uint32_t)c1;
                if (c1 >= bins) raise_status(status, CSA_E_INVALID, p1);
            }
        }
    }
}

// LDS row of the ordered pass: the bins, one spare entry, odd length
__host__ __device__ inline int64_t whist_row_stride(int64_t bins) { return (bins + 1) | 1; }

template <bool kLds>
__global__ __launch_bounds__(kWhSlab) void whist_sum_kernel(const uint32_t *__restrict__ counts, uint64_t n_panels,
                                                            const double *__restrict__ weights, int n_groups,
                                                            int bins, int slab, int accumulate, double *hist) {
    extern __shared__ double s_dyn[];
    double *s_w = s_dyn;              // [kWhChunk]
    double *s_row = s_dyn + kWhChunk;  // [slab][whist_row_stride(bins)] when kLds
    const int lane = threadIdx.x;
    const int g0 = (int)blockIdx.x * slab;
    const int ng = min(slab, n_groups - g0);
    const int stride = (int)whist_row_stride(bins);
    unsigned long long *hbits = reinterpret_cast<unsigned long long *>(hist);
    unsigned long long *sbits = reinterpret_cast<unsigned long long *>(s_row);

    if (kLds) {  // rows move as 64-bit words: stored bits (a -0.0, a NaN payload) survive
        for (int e = lane; e < ng * bins; e += kWhSlab) {
            const int j = e / bins, c = e - j * bins;
            sbits[j * stride + c] = accumulate ? hbits[(size_t)(g0 + j) * (size_t)bins + c] : 0ull;
        }
    }
    __syncthreads();

    // A lane without a group (lane >= ng) reads a valid count and adds nothing: its limit is 0.  In LDS
    // every add that must not count -- no group, a count no bin has -- goes to the row's spare entry
    // `bins`, which is never stored (lanes past the slab share the spare entries of its rows); on d_hist
    // there is no such entry and the store is predicated.
    const bool active = lane < ng;
    const uint32_t lim = active ? (uint32_t)bins : 0u;
    const uint32_t sink = kLds ? (uint32_t)bins : 0u;
    const uint32_t goff = (uint32_t)g0 + (active ? (uint32_t)lane : 0u);
    double *row = kLds ? s_row + (size_t)(lane & (slab - 1)) * stride : hist + (size_t)goff * (size_t)bins;

    auto fetch = [&](uint32_t(&c)[kWhUnroll], uint64_t p) {
        const uint32_t *b = counts + p * (uint64_t)n_groups;  // wave-uniform; the lane's offset is goff
#pragma unroll
        for (int i = 0; i < kWhUnroll; ++i) {
            c[i] = b[goff];
            b += n_groups;
        }
    };
    auto process = [&](const uint32_t(&cnt)[kWhUnroll], uint64_t p) {
        const int off = (int)(p & (uint64_t)(kWhChunk - 1));
        if (off == 0) {  // the next kWhChunk weights
            __syncthreads();
            for (int e = lane; e < kWhChunk; e += kWhSlab) s_w[e] = p + e < n_panels ? weights[p + e] : 0.0;
            __syncthreads();
        }
#pragma unroll
        for (int i0 = 0; i0 < kWhUnroll; i0 += kWhBlock) {
            // kWhBlock panels at once: their entries are read together (one LDS latency, not one per
            // panel), then added to in ascending p.  A panel whose entry an earlier panel of the block
            // also hit takes that panel's sum, not the stale read, so every entry still sees one add
            // per panel in order; the stores follow in order, the last one to an entry standing.
            uint32_t c[kWhBlock], idx[kWhBlock];
            double v[kWhBlock];
#pragma unroll
            for (int j = 0; j < kWhBlock; ++j) {
                c[j] = cnt[i0 + j];
                idx[j] = c[j] < lim ? c[j] : sink;
                v[j] = row[idx[j]];
            }
#pragma unroll
            for (int j = 0; j < kWhBlock; ++j) {
                double x = v[j];
#pragma unroll
                for (int h = 0; h < j; ++h)  // (raw counts: one that no bin has never equals one that a bin has)
                    if (c[h] == c[j]) x = v[h];  // v[h] is panel h's sum by now; the latest h wins
                v[j] = x + s_w[off + i0 + j];
            }
#pragma unroll
            for (int j = 0; j < kWhBlock; ++j)
                if (kLds || c[j] < lim) row[idx[j]] = v[j];
        }
    };

    // whole blocks of kWhUnroll panels, their counts in two register sets: one in flight, one being added
    const uint64_t nfull = n_panels - n_panels % kWhUnroll;
    uint32_t ca[kWhUnroll], cb[kWhUnroll];
    if (nfull) fetch(ca, 0);
    for (uint64_t p = 0; p < nfull; p += 2 * kWhUnroll) {
        const bool second = p + kWhUnroll < nfull;
        if (second) fetch(cb, p + kWhUnroll);
        process(ca, p);
        if (second) {
            if (p + 2 * kWhUnroll < nfull) fetch(ca, p + 2 * kWhUnroll);
            process(cb, p + kWhUnroll);
        }
    }
    for (uint64_t p = nfull; p < n_panels; ++p) {  // the last n_panels % kWhUnroll, one at a time
        const uint32_t c = counts[p * (uint64_t)n_groups + goff];
        const double w = weights[p];
        if (c < lim) row[c] += w;
    }

    if (kLds) {
        __syncthreads();
        for (int e = lane; e < ng * bins; e += kWhSlab) {
            const int j = e / bins, c = e - j * bins;
            if (j < ng && c < bins) hbits[(size_t)(g0 + j) * (size_t)bins + c] = sbits[j * stride + c];
        }
    }
}
