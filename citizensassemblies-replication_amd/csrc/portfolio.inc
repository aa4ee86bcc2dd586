// portfolio.inc -- portfolio_pairs_kernel: the LEXIMIN / XMIN analysis side (analysis.py:194-228).
// Included by csa_legacy.hip inside its anonymous namespace.
//
// After the solver returns (portfolio, probabilities), the reference adds every panel's probability to
// each of its k(k-1)/2 pairs (PairHistogram.add_portfolio_of_panels_to_histogram, analysis.py:90-95)
// and to each of its members (selection_probs, analysis.py:204-207), panel after panel.  Every value
// is therefore a float64 sum taken IN PORTFOLIO ORDER, and float64 addition does not associate: the
// same sum in another order differs in the last bits for thousands of pairs.  This kernel is the
// ordered weighted X^T D X that reproduces those bits.
//
// Contract, per pair (i, j) with i <= j (i == j is the per-person value): start from +0.0 (or from the
// stored value when accumulating) and add w[p] for every panel p that holds both agents, in ASCENDING
// p, one plain IEEE float64 add each.  One thread owns a pair for the whole panel range: no tree
// reduction, no split of the panels over threads or workgroups, no atomics on the values.  The build
// has no -ffast-math (see _native.build) and must not get it: reassociation would break the contract;
// there is no multiply to contract into an FMA.
//
// Shape: one 256-thread workgroup per 64 x 64 tile of the upper triangle; thread (ty, tx) owns the
// 4 x 4 block rows 4 ty .., columns 4 tx .. -- 16 float64 accumulators.  The panel planes (the XT
// layout of csa_transpose_count_async: one uint32 = one agent over 32 panels) are walked in order,
// kPfPlanes at a time staged in LDS with their weights: per plane a thread reads its 4 row words and
// 4 column words as two 16-byte LDS reads (row reads broadcast inside a 16-lane group, column reads
// cover one 256-byte bank row: conflict-free).  On a diagonal tile the row words are the column words,
// so the block's diagonal entries see m = x_i & x_i = x_i and ARE the per-person sums; 4 x 4 blocks
// wholly below the diagonal clear their row words and add nothing.
//
// The bit loop visits only the panels present in both words (while (m) { b = lowest set bit; ... }):
// at LEGACY densities (k / n of 2-6 %) nearly every AND is zero.  The branch-free alternative, adding
// a selected -0.0 for absent panels (the neutral addend must be MINUS zero: (-0.0) + (+0.0) would flip
// a stored -0.0), gave the same bits and was 3x slower at sf_e and 14x at n = 8192 (DESIGN 4.9), so it
// is not kept.  A plane in which no lane of the wavefront has a common bit is skipped with a
// wave-uniform test.
constexpr int kPfTile = 64;
constexpr int kPfThreads = 256;
constexpr int kPfPlanes = 32;  // planes staged per barrier pair = 1024 panels: 16 KB of bits + 8 KB of weights

__device__ __forceinline__ uint64_t pf_upper_index(int i, int j, int n) {  // i < j: PairHistogram's order
    return (uint64_t)i * (uint64_t)(2 * (int64_t)n - i - 1) / 2 + (uint64_t)(j - i - 1);
}

__global__ __launch_bounds__(kPfThreads) void portfolio_pairs_kernel(const uint32_t *__restrict__ xt32,
                                                                     uint64_t n_panels, int n, int npad,
                                                                     const double *__restrict__ weights,
                                                                     double *__restrict__ upper,
                                                                     double *__restrict__ alloc, int accumulate) {
    __shared__ __attribute__((aligned(16))) uint32_t s_row[kPfPlanes][kPfTile];
    __shared__ __attribute__((aligned(16))) uint32_t s_col[kPfPlanes][kPfTile];
    __shared__ __attribute__((aligned(16))) double s_w[kPfPlanes * 32];

    // blockIdx.x -> tile (ti, tj), ti <= tj, row-major over the upper triangle of nt x nt tiles
    const int nt = (n + kPfTile - 1) / kPfTile;
    int ti = 0;
    unsigned rem = blockIdx.x;
    while (rem >= (unsigned)(nt - ti)) {
        rem -= (unsigned)(nt - ti);
        ++ti;
    }
    const int tj = ti + (int)rem;
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int i0 = ti * kPfTile + 4 * ty, j0 = tj * kPfTile + 4 * tx;
    const bool below = ti == tj && ty > tx;  // the whole 4 x 4 block lies under the diagonal

    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + a, j = j0 + b;
            double v = 0.0;
            if (accumulate && j < n) {
                if (i < j) {
                    if (upper) v = upper[pf_upper_index(i, j, n)];
                } else if (i == j && alloc) {
                    v = alloc[i];
                }
            }
            acc[a][b] = v;
        }

    const uint64_t nplanes = (n_panels + 31) / 32;
    for (uint64_t q0 = 0; q0 < nplanes; q0 += kPfPlanes) {
        const int np = (int)min((uint64_t)kPfPlanes, nplanes - q0);
        __syncthreads();  // every wave is done with the previous chunk
        for (int pl = t >> 6; pl < np; pl += kPfThreads / 64) {
            const uint64_t q = q0 + pl;
            // bits past n_panels in the last plane are not panels (the transpose leaves zeros there;
            // masked regardless)
            const uint64_t left = n_panels - q * 32;
            const uint32_t keep = left >= 32 ? 0xFFFFFFFFu : ((1u << (unsigned)left) - 1u);
            const uint32_t *src = xt32 + q * (uint64_t)npad;
            s_row[pl][t & 63] = src[ti * kPfTile + (t & 63)] & keep;
            s_col[pl][t & 63] = src[tj * kPfTile + (t & 63)] & keep;
        }
        for (int e = t; e < np * 32; e += kPfThreads) {
            const uint64_t p = q0 * 32 + (uint64_t)e;
            s_w[e] = p < n_panels ? weights[p] : 0.0;
        }
        __syncthreads();
        for (int pl = 0; pl < np; ++pl) {
            uint4 r = *reinterpret_cast<const uint4 *>(&s_row[pl][4 * ty]);
            const uint4 c = *reinterpret_cast<const uint4 *>(&s_col[pl][4 * tx]);
            if (below) r = make_uint4(0u, 0u, 0u, 0u);
            const uint32_t xi[4] = {r.x, r.y, r.z, r.w}, xj[4] = {c.x, c.y, c.z, c.w};
            // wave-uniform skip: no lane has a row word and a column word with a common panel
            if (!__any(((r.x | r.y | r.z | r.w) & (c.x | c.y | c.z | c.w)) != 0u)) continue;
            const double *wp = s_w + pl * 32;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    uint32_t m = xi[a] & xj[b];
                    while (m) {  // ascending bit = ascending panel
                        const int bit = __ffs((int)m) - 1;
                        m &= m - 1u;
                        acc[a][b] += wp[bit];
                    }
                }
        }
    }

#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + a, j = j0 + b;
            if (j < n) {
                if (i < j) {
                    if (upper) upper[pf_upper_index(i, j, n)] = acc[a][b];
                } else if (i == j && alloc) {
                    alloc[i] = acc[a][b];
                }
            }
        }
}
