// rows_nash.inc -- the Nash-welfare lottery over a table of drawn panels: the row probabilities p that maximise
// the product (the geometric mean) of the agents' selection probabilities pi = M^T p, M the table's membership
// matrix, over the agents some valid row holds.  Cover's multiplicative iteration p_d <- p_d G_d / m with
// G_d = the sum of 1 / pi_i over row d's members and m = the number of held agents keeps the sum of p at 1, raises
// the objective monotonically and has the optimum as its fixed point; (max_d G_d / m) * (sum of p) bounds
// optimum / current geometric mean from above (Jensen), so every round carries a certificate.  Included by
// csa_legacy.hip inside an anonymous namespace, after rows_maximin.inc, last in the code object; the kernels are
// templates of an unused parameter for the reason rows_price.inc gives.
//
// Table, length, padded weights, the order "best" (rp_beats) and the slab are rows_price.inc's, the first-holder
// pass is rp_first_holder_kernel and the score pass IS rp_score_kernel, both unchanged: with the weights 1 / pi
// its scores are G.  What is new is the transposed product, the per-agent marginal of a weighted table, in an
// order a host loop reproduces.  All arithmetic is float64; fp contraction is off wherever a product or a
// quotient feeds another operation.
//
//   rn_start_kernel     p[d] = (double)mult[d] / (double)total for the valid rows, or 1.0 / (double)D with a NULL
//                       mult: one IEEE division each.  Nothing past the length is written.
//   rn_marginal_kernel  the hot pass.  The table is cut into tiles of kRnTile consecutive rows; part[b][i] = the
//                       sum from +0.0, in ascending row order, of p[d] over tile b's valid rows whose bit i is
//                       set -- one rounded add per holder, a row that does not hold i adds nothing --, and
//                       psum_part[b] = the same sum over all the tile's valid rows.  One wave per (tile,
//                       kRnWords consecutive row words), an accumulator per word, lane l of word j = agent
//                       64 j + l; a workgroup is kRnWaves such waves of one tile.  A row's words and p[d] are
//                       wave-uniform: scalar loads (32 bytes a row), kRnBatch rows in flight before the first
//                       add, and a word itself is the lane mask of its add (no bit test on the VALU): one
//                       v_add_f64 and a 64-bit select per row, word and 64 agents.  No LDS.  The wave of word 0
//                       also sums p.  A row's last words take the narrower forms, so nothing past a row is
//                       loaded; a tile past the length writes nothing and a row past the length is never loaded.
//   rn_finish_kernel    pi[i] = the sum over ascending valid tiles b, from +0.0, of part[b][i]; marginals[i] =
//                       pi[i] for i < n.  With first holders: inv[i] = 1.0 / pi[i] (IEEE division) where
//                       first[i] names a row, else +0.0, for all 64 W padded entries.  The last workgroup instead
//                       adds psum = the psum_part of the valid tiles in ascending order from +0.0.  A round over
//                       an empty table writes nothing.
//   rn_held_kernel      one workgroup, once per call after the first-holder pass: m = how many first[i] name a row.
//   rn_step_kernel      p[d] = p[d] * (scores[d] / (double)m) for the valid rows: one division, then one
//                       rounded multiply.
//   rn_bound_kernel     one workgroup after a score pass: U = the slab's best; ratio = (U / (double)m) * psum, one
//                       division then one rounded multiply; state = (bits of ratio, rounds done, best row, bits
//                       of psum), rounds done = 0 at the start, else + 1.  An empty table: at the start (+inf, 0,
//                       kRpNone, +0.0), else nothing.
//
// A table with valid rows is assumed to hold somebody (m > 0; a panel has k >= 1 members): rn_step_kernel and
// rn_bound_kernel divide by m unguarded, as the header says.
//
// Scratch (8-byte aligned): the slab, 16 bytes per kRpTile rows | part, 64 W float64 per kRnTile rows | psum_part,
// a float64 per kRnTile rows | inv, 64 W float64 | first holders, 64 W uint32 | psum (float64) and m (uint64).
// csa_rows_marginals_async uses part | psum_part alone.  Every index into it, the rows, p and the scores is below
// a size the host passed: a row is < min(*d_len, cap), a tile < rn_tiles(cap), a word < W.
constexpr int kRnTile = 1024;    // rows per marginal tile: the unit of the summation order
constexpr int kRnWords = 4;      // row words per wave: one 32-byte scalar load a row, one accumulator a word
constexpr int kRnWaves = 8;      // waves per workgroup: 32 consecutive words of one tile
constexpr int kRnBatch = 8;      // rows whose words and p a wave loads before it adds
static_assert(kRnWords == 4, "rn_marginal_kernel dispatches on 1 .. 4 words");
constexpr int kRnThreads = 64 * kRnWaves;
constexpr size_t kRnTail = 16;   // psum and m

__host__ __device__ inline uint64_t rn_tiles(uint64_t rows) { return (rows + kRnTile - 1) / kRnTile; }
__host__ inline uint64_t rn_part_bytes(uint64_t cap, int W) { return rn_tiles(cap) * ((uint64_t)64 * W + 1) * 8; }
__host__ inline uint64_t rn_scratch_bytes(uint64_t cap, int W) {
    return 16 * rp_blocks(cap) + rn_part_bytes(cap, W) + (uint64_t)64 * W * 8 + (uint64_t)64 * W * 4 + kRnTail;
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rn_start_kernel(const unsigned long long *__restrict__ d_len,
                                                              uint64_t cap, const uint32_t *__restrict__ mult,
                                                              uint64_t total, double *__restrict__ prob) {
    const uint64_t len = min((uint64_t)*d_len, cap);
    const uint64_t d = (uint64_t)blockIdx.x * kRpThreads + threadIdx.x;
    if (d >= len) return;
    prob[d] = mult ? (double)mult[d] / (double)total : 1.0 / (double)len;
}

// one wave: the ordered, masked sums of p over cnt rows whose words are W apart, for G consecutive words at r (one
// accumulator each); with kSum also the plain sum
template <int G, bool kSum>
__device__ __forceinline__ void rn_wave_sums(const uint64_t *__restrict__ r, const double *__restrict__ p, int cnt,
                                             int W, double *__restrict__ out, double &all) {
    double acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = 0.0;
    int d = 0;
    for (; d + kRnBatch <= cnt; d += kRnBatch) {
        uint64_t w[kRnBatch][G];
        double v[kRnBatch];
#pragma unroll
        for (int u = 0; u < kRnBatch; ++u) {
#pragma unroll
            for (int g = 0; g < G; ++g) w[u][g] = r[(size_t)(d + u) * W + g];
            v[u] = p[d + u];
        }
        // every load of the batch is in flight before the first add: left alone, the scheduler trades that for
        // fewer scalar registers and the loads queue behind one another
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kRnBatch; ++u) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double t = acc[g] + v[u];
                acc[g] = __builtin_amdgcn_inverse_ballot_w64(w[u][g]) ? t : acc[g];   // lane l: bit l of the word
            }
            if (kSum) all = all + v[u];
        }
    }
    for (; d < cnt; ++d) {
        const double v = p[d];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double t = acc[g] + v;
            acc[g] = __builtin_amdgcn_inverse_ballot_w64(r[(size_t)d * W + g]) ? t : acc[g];
        }
        if (kSum) all = all + v;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) out[64 * g] = acc[g];
}

template <int kLate = 0>
__global__ __launch_bounds__(kRnThreads) void rn_marginal_kernel(const uint64_t *__restrict__ rows,
                                                                 const unsigned long long *__restrict__ d_len,
                                                                 uint64_t cap, int W, const double *__restrict__ prob,
                                                                 double *__restrict__ part,
                                                                 double *__restrict__ psum_part) {
    const uint64_t len = min((uint64_t)*d_len, cap);
    const uint64_t row0 = (uint64_t)blockIdx.x * kRnTile;
    // the first word of this wave: the same in every lane, and said so, so that the loads below are scalar
    const int j = __builtin_amdgcn_readfirstlane((int)((blockIdx.y * kRnWaves + (threadIdx.x >> 6)) * kRnWords));
    if (row0 >= len || j >= W) return;   // the whole wave
    const int cnt = (int)min((uint64_t)kRnTile, len - row0);
    const uint64_t *r = rows + row0 * W + j;
    const double *p = prob + row0;
    double *out = part + ((uint64_t)blockIdx.x * W + j) * 64 + (threadIdx.x & 63);
    double all = 0.0;
    const int G = min(kRnWords, W - j);   // a row's last words: never a load past the row
    if (j == 0) {
        if (G == 4) rn_wave_sums<4, true>(r, p, cnt, W, out, all);
        else if (G == 3) rn_wave_sums<3, true>(r, p, cnt, W, out, all);
        else if (G == 2) rn_wave_sums<2, true>(r, p, cnt, W, out, all);
        else rn_wave_sums<1, true>(r, p, cnt, W, out, all);
        if ((threadIdx.x & 63) == 0) psum_part[blockIdx.x] = all;
    } else {
        if (G == 4) rn_wave_sums<4, false>(r, p, cnt, W, out, all);
        else if (G == 3) rn_wave_sums<3, false>(r, p, cnt, W, out, all);
        else if (G == 2) rn_wave_sums<2, false>(r, p, cnt, W, out, all);
        else rn_wave_sums<1, false>(r, p, cnt, W, out, all);
    }
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rn_held_kernel(const uint32_t *__restrict__ first, int n,
                                                             uint64_t *__restrict__ m_word) {
    __shared__ unsigned s_held[kRpThreads / 64];
    unsigned held = 0;
    for (int i = threadIdx.x; i < n; i += kRpThreads) held += first[i] != kRpNoRow;
    for (int d = 32; d > 0; d >>= 1) held += __shfl_down(held, d);
    if ((threadIdx.x & 63) == 0) s_held[threadIdx.x >> 6] = held;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int q = 1; q < kRpThreads / 64; ++q) held += s_held[q];
    *m_word = held;
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rn_finish_kernel(const unsigned long long *__restrict__ d_len,
                                                               uint64_t cap, int W, int n, int empty_too,
                                                               const double *__restrict__ part,
                                                               const double *__restrict__ psum_part,
                                                               const uint32_t *__restrict__ first,
                                                               double *__restrict__ marginals, double *__restrict__ inv,
                                                               double *__restrict__ psum) {
    const uint64_t tiles = rn_tiles(min((uint64_t)*d_len, cap));
    if (!tiles && !empty_too) return;   // a round over an empty table changes nothing
    const size_t stride = (size_t)64 * W;
    if (blockIdx.x + 1 == gridDim.x) {   // the last workgroup: the sum of p
        if (threadIdx.x != 0) return;
        double a = 0.0;
#pragma unroll 8
        for (uint64_t b = 0; b < tiles; ++b) a = a + psum_part[b];
        *psum = a;
        return;
    }
    const size_t i = (size_t)blockIdx.x * kRpThreads + threadIdx.x;
    if (i >= stride) return;
    double a = 0.0;
#pragma unroll 16
    for (uint64_t b = 0; b < tiles; ++b) a = a + part[b * stride + i];
    if (i < (size_t)n) marginals[i] = a;
    if (inv) inv[i] = (i < (size_t)n && first[i] != kRpNoRow) ? 1.0 / a : 0.0;
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rn_step_kernel(const unsigned long long *__restrict__ d_len,
                                                             uint64_t cap, const double *__restrict__ scores,
                                                             const uint64_t *__restrict__ m_word,
                                                             double *__restrict__ prob) {
#pragma clang fp contract(off)
    const uint64_t len = min((uint64_t)*d_len, cap);
    const uint64_t d = (uint64_t)blockIdx.x * kRpThreads + threadIdx.x;
    if (d >= len) return;
    const double g = scores[d] / (double)*m_word;   // rounded before the multiply: contraction is off
    prob[d] = prob[d] * g;
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rn_bound_kernel(const uint64_t *__restrict__ slab, uint64_t n_blocks,
                                                              const double *__restrict__ psum,
                                                              const uint64_t *__restrict__ m_word, int start,
                                                              uint64_t *__restrict__ state) {
#pragma clang fp contract(off)
    RP_LDS;
    uint64_t *s_row = reinterpret_cast<uint64_t *>(rp_lds);
    double *s_score = reinterpret_cast<double *>(s_row + kRpThreads / 64);
    uint64_t row;
    double score;
    rp_slab_best(slab, n_blocks, row, score, s_row, s_score);
    if (threadIdx.x != 0) return;
    if (row == kRpNone) {
        if (start) {
            state[0] = 0x7FF0000000000000ull;
            state[1] = 0ull;
            state[2] = kRpNone;
            state[3] = 0ull;
        }
        return;
    }
    const double g = score / (double)*m_word;
    const double s = *psum;
    const double ratio = g * s;
    state[0] = (uint64_t)__double_as_longlong(ratio);
    state[1] = start ? 0ull : state[1] + 1ull;
    state[2] = row;
    state[3] = (uint64_t)__double_as_longlong(s);
}
