// rows_price.inc -- a weight per agent against a table of panels: the weight sum of every row, the best row,
// rounds of the multiplicative-weights cover over the table, and the lowest row holding each agent.  This is
// the question both loops of the reference's column generation put to its ILP (xmin.py:229-290, the
// multiplicative-weights stage; xmin.py:410-440, the dual values), answered over panels that were drawn.
// Included by csa_legacy.hip inside an anonymous namespace, after rows_join.inc; the kernels are templates of
// an unused parameter for the reason given in multiplicity_exchange.inc's "Layout": every kernel that existed
// keeps its offset in the code object.
//
// Rows are uint64[cap][W], agent p = bit p & 63 of word p >> 6, padding bits zero; the valid length is
// min(*d_len, cap), read on the device, and a row past it is never loaded.  Weights sit in LDS padded to
// 64 * W entries of +0.0, so a stray padding bit adds 0.0 and reads inside the array.
//
//   rp_score_kernel         score[d] = the sum of w[i] over the set bits of row d: float64, from +0.0, one
//                           rounded add per member in ASCENDING agent index -- no tree, no split of a row over
//                           lanes, no multiply (nothing to contract), the discipline of portfolio_pairs_kernel
//                           and whist_sum_kernel, so a host loop gives the same bits.  One row per lane; a wave
//                           stages its 64 rows kRpSeg words at a time in LDS (coalesced 128-byte runs in, rows
//                           of odd stride out, so the lanes of a half-wave read distinct banks) and each lane
//                           walks the set bits of its words.  The workgroup's best (row, score) goes to slab
//                           entry blockIdx.x; a workgroup past the length writes (kRpNone, -inf).
//   rp_best_kernel          one workgroup: the slab's best into d_best[2] = (index_base + row, score bits).
//   rp_round_kernel         one workgroup: one multiplicative-weights round after a score pass (see below).
//   rp_first_holder_kernel  first[i] = the lowest row holding agent i: atomicMin into an LDS array per
//                           workgroup over a grid-stride walk of the table's words, one flush of the entries
//                           that were reached (first[] pre-filled with 0xFFFFFFFF by the enqueue).
//
// Best.  a beats b when a's score > b's as float64 values, or neither is greater and a's row is lower; a
// kRpNone row never beats anything.  Without NaNs that is a total order, so the lane / wave / slab tree
// gives what a scan in ascending row order gives: the first row holding the maximum.  A sum that starts at
// +0.0 is never -0.0, so equal scores are equal bits.
//
// Round (the order of xmin.py:251-266).  p = the slab's best; picks[r] = p; w[i] *= 0.8 for the members of
// row p; s = the lane-strided sum of w -- partial[l] = sum over ascending j of w[64 j + l] from +0.0 over
// the padded array, then s = the sum over ascending l of partial[l] from +0.0 --; f = n / s; w[i] *= f for
// all i; then, if chosen[p] was set, w[i] = 0.9 * w[i] + 0.1 with the product and the sum rounded apart
// (fp contraction is off in that kernel), else chosen[p] = 1.  An empty table writes the pick 0xFFFFFFFF
// and leaves the weights alone.  T rounds are 2 T plain launches on one stream: nothing spans workgroups
// inside a launch, so nothing needs them co-resident.
constexpr int kRpThreads = 256;
constexpr int kRpTile = kRpThreads;        // rp_score_kernel: rows per workgroup, one per thread
constexpr int kRpSeg = 16;                 // row words a wave stages per pass (128-byte runs)
constexpr int kRpSegStride = kRpSeg + 1;   // odd: ds_read_b64 of 32 lanes on 32 bank pairs
constexpr uint64_t kRpNone = 0xFFFFFFFFFFFFFFFFull;
constexpr uint32_t kRpNoRow = 0xFFFFFFFFu;

// All LDS is one dynamic region, 16-byte aligned, every part a multiple of 16 bytes: the weights (or the
// first-holder words) lead, the staged tiles follow, the reductions' few words come last.
constexpr size_t kRpBestLds = 2 * (kRpThreads / 64) * 8;   // rp_block_best: a (row, score) per wave
__host__ __device__ inline size_t rp_tiles_lds() { return (size_t)kRpThreads * kRpSegStride * 8; }
__host__ __device__ inline size_t rp_score_lds(int W) { return (size_t)64 * W * 8 + rp_tiles_lds() + kRpBestLds; }
__host__ __device__ inline size_t rp_round_lds(int W) { return (size_t)64 * W * 8 + 64 * 8 + kRpBestLds + 32; }
#define RP_LDS extern __shared__ __attribute__((aligned(16))) unsigned char rp_lds[]

__device__ __forceinline__ double rp_minus_inf() { return __longlong_as_double((long long)0xFFF0000000000000ull); }

__device__ __forceinline__ bool rp_beats(uint64_t ra, double sa, uint64_t rb, double sb) {
    if (ra == kRpNone) return false;
    if (rb == kRpNone) return true;
    return sa > sb || (!(sb > sa) && ra < rb);
}

// the workgroup's best of (row, score) into thread 0's
__device__ __forceinline__ void rp_block_best(uint64_t &row, double &score, uint64_t *s_row, double *s_score) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t r2 = (uint64_t)__shfl_down((unsigned long long)row, d);
        const double s2 = __shfl_down(score, d);
        if (lane + d < 64 && rp_beats(r2, s2, row, score)) row = r2, score = s2;
    }
    if (lane == 0) s_row[wave] = row, s_score[wave] = score;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < kRpThreads / 64; ++q)
            if (rp_beats(s_row[q], s_score[q], row, score)) row = s_row[q], score = s_score[q];
}

// thread 0: the best of the n_blocks slab entries (row, score bits)
__device__ __forceinline__ void rp_slab_best(const uint64_t *__restrict__ slab, uint64_t n_blocks, uint64_t &row,
                                             double &score, uint64_t *s_row, double *s_score) {
    row = kRpNone, score = rp_minus_inf();
    for (uint64_t b = threadIdx.x; b < n_blocks; b += kRpThreads) {
        const uint64_t r2 = slab[2 * b];
        const double s2 = __longlong_as_double((long long)slab[2 * b + 1]);
        if (rp_beats(r2, s2, row, score)) row = r2, score = s2;
    }
    rp_block_best(row, score, s_row, s_score);
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rp_score_kernel(const uint64_t *__restrict__ rows,
                                                              const unsigned long long *__restrict__ d_len,
                                                              uint64_t cap, int W, int n,
                                                              const double *__restrict__ weights,
                                                              double *__restrict__ scores, uint64_t *__restrict__ slab) {
    RP_LDS;
    double *s_w = reinterpret_cast<double *>(rp_lds);                                  // [64 * W]
    uint64_t *s_tiles = reinterpret_cast<uint64_t *>(rp_lds + (size_t)64 * W * 8);     // [kRpThreads][kRpSegStride]
    uint64_t *s_row = reinterpret_cast<uint64_t *>(rp_lds + (size_t)64 * W * 8 + rp_tiles_lds());
    double *s_score = reinterpret_cast<double *>(s_row + kRpThreads / 64);
    const uint64_t len = min((uint64_t)*d_len, cap);
    const uint64_t row0 = (uint64_t)blockIdx.x * kRpTile;
    if (row0 >= len) {   // the whole workgroup
        if (threadIdx.x == 0) {
            slab[2 * (uint64_t)blockIdx.x] = kRpNone;
            slab[2 * (uint64_t)blockIdx.x + 1] = 0xFFF0000000000000ull;
        }
        return;
    }
    for (int i = threadIdx.x; i < 64 * W; i += kRpThreads) s_w[i] = i < n ? weights[i] : 0.0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *tile = s_tiles + (size_t)wave * 64 * kRpSegStride;
    const uint64_t wave_row0 = row0 + (uint64_t)wave * 64, my = wave_row0 + lane;
    const uint64_t *mine = tile + lane * kRpSegStride;
    double s = 0.0;
    for (int c0 = 0; c0 < W; c0 += kRpSeg) {
        const int C = min(kRpSeg, W - c0);
        for (int e = lane; e < 64 * C; e += 64) {
            const int r = C == kRpSeg ? e / kRpSeg : e / C, w = e - r * C;
            const uint64_t g = wave_row0 + r;
            tile[r * kRpSegStride + w] = g < len ? rows[g * W + c0 + w] : 0ull;
        }
        __syncthreads();   // the staged words (and, the first time, the weights)
        for (int w = 0; w < C; ++w) {
            uint64_t x = mine[w];
            const double *wb = s_w + 64 * (c0 + w);
            while (x) {
                s = s + wb[__ffsll((unsigned long long)x) - 1];
                x &= x - 1;
            }
        }
        __syncthreads();   // before the next pass overwrites the tile
    }
    const bool valid = my < len;
    if (valid && scores) scores[my] = s;
    uint64_t row = valid ? my : kRpNone;
    rp_block_best(row, s, s_row, s_score);
    if (threadIdx.x == 0) {
        slab[2 * (uint64_t)blockIdx.x] = row;
        slab[2 * (uint64_t)blockIdx.x + 1] = (uint64_t)__double_as_longlong(s);
    }
}

// d_best = (index_base + row, score bits); accumulating, the stored pair yields only to a strictly greater
// score, or when it holds kRpNone
template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rp_best_kernel(const uint64_t *__restrict__ slab, uint64_t n_blocks,
                                                             uint64_t index_base, int accumulate,
                                                             uint64_t *__restrict__ best) {
    RP_LDS;
    uint64_t *s_row = reinterpret_cast<uint64_t *>(rp_lds);
    double *s_score = reinterpret_cast<double *>(s_row + kRpThreads / 64);
    uint64_t row;
    double score;
    rp_slab_best(slab, n_blocks, row, score, s_row, s_score);
    if (threadIdx.x != 0) return;
    if (accumulate) {
        if (row == kRpNone) return;
        const uint64_t old = best[0];
        if (old != kRpNone && !(score > __longlong_as_double((long long)best[1]))) return;
    }
    best[0] = row == kRpNone ? kRpNone : index_base + row;
    best[1] = (uint64_t)__double_as_longlong(row == kRpNone ? rp_minus_inf() : score);
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rp_round_kernel(const uint64_t *__restrict__ rows, int W, int n,
                                                              const uint64_t *__restrict__ slab, uint64_t n_blocks,
                                                              double *__restrict__ weights, uint8_t *__restrict__ chosen,
                                                              uint32_t *__restrict__ picks,
                                                              double *__restrict__ pick_scores, uint32_t round) {
#pragma clang fp contract(off)
    RP_LDS;
    double *s_w = reinterpret_cast<double *>(rp_lds);   // [64 * W]
    double *s_part = s_w + (size_t)64 * W;              // [64]
    uint64_t *s_row = reinterpret_cast<uint64_t *>(s_part + 64);
    double *s_score = reinterpret_cast<double *>(s_row + kRpThreads / 64);
    double &s_f = s_score[kRpThreads / 64];
    uint64_t &s_pick = reinterpret_cast<uint64_t *>(s_score)[kRpThreads / 64 + 1];
    uint64_t &s_repeat = reinterpret_cast<uint64_t *>(s_score)[kRpThreads / 64 + 2];
    uint64_t row;
    double score;
    rp_slab_best(slab, n_blocks, row, score, s_row, s_score);
    if (threadIdx.x == 0) {
        s_pick = row;
        picks[round] = row == kRpNone ? kRpNoRow : (uint32_t)row;   // rows < cap < 2^32 - 1
        if (pick_scores) pick_scores[round] = row == kRpNone ? rp_minus_inf() : score;
        if (row != kRpNone) {
            s_repeat = chosen[row];
            chosen[row] = 1;
        }
    }
    __syncthreads();
    const uint64_t p = s_pick;
    if (p == kRpNone) return;   // the whole workgroup: an empty table leaves the weights alone
    const uint64_t *prow = rows + p * W;
    for (int i = threadIdx.x; i < 64 * W; i += kRpThreads) {
        double v = 0.0;
        if (i < n) {
            v = weights[i];
            if ((prow[i >> 6] >> (i & 63)) & 1) v = v * 0.8;
        }
        s_w[i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        double a = 0.0;
        for (int j = 0; j < W; ++j) a = a + s_w[64 * j + threadIdx.x];
        s_part[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int l = 0; l < 64; ++l) a = a + s_part[l];
        s_f = (double)n / a;
    }
    __syncthreads();
    const double f = s_f;
    const bool repeat = s_repeat != 0;
    for (int i = threadIdx.x; i < n; i += kRpThreads) {
        double v = s_w[i] * f;
        if (repeat) {
            const double t = 0.9 * v;   // rounded before the add: contraction is off
            v = t + 0.1;
        }
        weights[i] = v;
    }
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rp_first_holder_kernel(const uint64_t *__restrict__ rows,
                                                                     const unsigned long long *__restrict__ d_len,
                                                                     uint64_t cap, int W, int n,
                                                                     uint32_t *__restrict__ first) {
    RP_LDS;
    uint32_t *s_first = reinterpret_cast<uint32_t *>(rp_lds);   // [64 * W]
    for (int i = threadIdx.x; i < 64 * W; i += kRpThreads) s_first[i] = kRpNoRow;
    __syncthreads();
    const uint64_t words = min((uint64_t)*d_len, cap) * W;
    const uint64_t step = (uint64_t)gridDim.x * kRpThreads;
    for (uint64_t g = (uint64_t)blockIdx.x * kRpThreads + threadIdx.x; g < words; g += step) {
        uint64_t x = rows[g];
        if (!x) continue;
        const uint64_t r = g / W;
        uint32_t *at = s_first + 64 * (int)(g - r * W);
        const uint32_t row = (uint32_t)r;   // cap < 2^32 - 1
        while (x) {
            const int b = __ffsll((unsigned long long)x) - 1;
            if (row < at[b]) atomicMin(at + b, row);   // the entries only fall: a stale read costs an atomic, no more
            x &= x - 1;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kRpThreads) {
        const uint32_t v = s_first[i];
        if (v != kRpNoRow) atomicMin(first + i, v);
    }
}

__host__ inline uint64_t rp_blocks(uint64_t cap) { return (cap + kRpTile - 1) / kRpTile; }
