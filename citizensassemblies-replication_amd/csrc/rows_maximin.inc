// rows_maximin.inc -- the maximin lottery over a table of drawn panels: the reference's _dual_leximin_stage
// with no fixed probabilities and P ranging over the table's rows (xmin.py:293-321, the first outer iteration
// of _expand_distribution_leximin), solved as a zero-sum game by multiplicative weights.  Each round picks the
// best row under the weights and shrinks its members' weights; how often each row was picked is a lottery
// over the rows (a lower bound on the optimum: the least cover / rounds), every normalised weight vector met
// is a dual point (an upper bound: the best score / the weights' sum).  Included by csa_legacy.hip inside an
// anonymous namespace, after rows_price.inc, last in the code object; the kernels are templates of an unused
// parameter for the reason rows_price.inc gives.
//
// Table, length, padded LDS weights, the order "best" (rp_beats) and the lane-strided sum are rows_price.inc's,
// and the fresh score pass IS rp_score_kernel, unchanged.  What is new is that a round changes only the weights
// of the picked row's k members, so between fresh passes a row's score changes only by the weights on its
// intersection with the picked row -- about k^2 / n agents, not k:
//
//   rm_start_kernel    one workgroup: w[i] = 1.0 where first[i] names a row, else +0.0; cover = 0; rounds done
//                      = 0; the lane-strided sum of w into the scratch's sum word.
//   rm_rescan_kernel   the slab from d_scores alone (a call that continues another owns no slab yet): entry
//                      blockIdx.x = the best (row, score) of its kRpTile rows.
//   rm_pick_kernel     one workgroup, one round: p = the slab's best; picks[r] = p; row_count[p] += 1;
//                      cover[i] += 1, v = w[i] * shrink, delta[i] = w[i] - v, w[i] = v for the members of row p
//                      (one rounded multiply, one rounded subtract: contraction is off), delta = +0.0 for
//                      everyone else; p into the scratch's pick word.  On a fresh round also s = the
//                      lane-strided sum of w, f = (double)n / s, w[i] *= f, and the lane-strided sum of the new
//                      w into the sum word.  An empty table: picks[r] = 0xFFFFFFFF, nothing else.
//   rm_update_kernel   the hot pass of a round that is not fresh: for every valid row d, t = the sum of
//                      delta[i] over the set bits of row_d & row_p in ascending i from +0.0, one rounded add
//                      each; scores[d] = scores[d] - t; the workgroup's best to the slab.  One row per lane;
//                      a wave stages its 64 rows kRpSeg words at a time in rp_score_kernel's tile layout, but
//                      on its own (no workgroup barrier in the loop) and one pass ahead in registers; delta
//                      (64 W float64) and row p's W words in LDS; a staging pass none of whose words row p
//                      touches is skipped whole (no loads), a word row p does not touch is skipped
//                      wave-uniformly.
//   rm_bound_kernel    one workgroup after a fresh score pass: U = the slab's best, u = U / the sum word
//                      (IEEE division); state = (upper, rounds done, best row, u) with upper = u at the start,
//                      else u if u < upper.  An empty table: at the start (+inf, 0, kRpNone, +inf), else
//                      nothing.
//
// Scratch (8-byte aligned): the slab, 16 bytes per kRpTile rows | delta, 64 W float64 | first holders, 64 W
// uint32 | the pick word (uint64) | the sum word (float64).  Every index into it, into the rows, the scores and
// the row counts is below a size the host passed: a pick is a slab row, a slab row is < min(*d_len, cap).
constexpr size_t kRmTail = 16;   // the pick word and the sum word
static_assert(kRpSeg == 16, "rm_update_kernel stages 4 rows x 16 words per instruction");

__host__ __device__ inline size_t rm_update_lds(int W) {
    return (size_t)64 * W * 8 + (size_t)((W + 1) & ~1) * 8 + rp_tiles_lds() + kRpBestLds;
}
__host__ __device__ inline size_t rm_pick_lds(int W) { return (size_t)64 * W * 8 + 64 * 8 + kRpBestLds + 32; }
__host__ inline uint64_t rm_scratch_bytes(uint64_t cap, int W) {
    return 16 * rp_blocks(cap) + (uint64_t)64 * W * 8 + (uint64_t)64 * W * 4 + kRmTail;
}

// orders a wave's LDS writes before its own later LDS reads (and the reverse): the LDS serves a wave's
// instructions in order, so program order is enough once the compiler keeps it
__device__ __forceinline__ void rm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the lane-strided sum of the 64 W padded weights in s_w into thread 0's return (all threads call)
__device__ __forceinline__ double rm_lane_sum(const double *s_w, double *s_part, int W) {
    if (threadIdx.x < 64) {
        double a = 0.0;
        for (int j = 0; j < W; ++j) a = a + s_w[64 * j + threadIdx.x];
        s_part[threadIdx.x] = a;
    }
    __syncthreads();
    double a = 0.0;
    if (threadIdx.x == 0)
        for (int l = 0; l < 64; ++l) a = a + s_part[l];
    return a;
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rm_start_kernel(const uint32_t *__restrict__ first, int W, int n,
                                                              double *__restrict__ weights,
                                                              uint32_t *__restrict__ cover, uint64_t *__restrict__ state,
                                                              double *__restrict__ sum_word) {
    RP_LDS;
    double *s_w = reinterpret_cast<double *>(rp_lds);   // [64 * W]
    double *s_part = s_w + (size_t)64 * W;              // [64]
    for (int i = threadIdx.x; i < 64 * W; i += kRpThreads) {
        double v = 0.0;
        if (i < n) {
            v = first[i] != kRpNoRow ? 1.0 : 0.0;
            weights[i] = v;
            cover[i] = 0u;
        }
        s_w[i] = v;
    }
    __syncthreads();
    const double s = rm_lane_sum(s_w, s_part, W);
    if (threadIdx.x == 0) {
        *sum_word = s;
        state[1] = 0ull;
    }
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rm_rescan_kernel(const unsigned long long *__restrict__ d_len,
                                                               uint64_t cap, const double *__restrict__ scores,
                                                               uint64_t *__restrict__ slab) {
    RP_LDS;
    uint64_t *s_row = reinterpret_cast<uint64_t *>(rp_lds);
    double *s_score = reinterpret_cast<double *>(s_row + kRpThreads / 64);
    const uint64_t len = min((uint64_t)*d_len, cap);
    const uint64_t my = (uint64_t)blockIdx.x * kRpTile + threadIdx.x;
    const bool valid = my < len;
    double s = valid ? scores[my] : rp_minus_inf();
    uint64_t row = valid ? my : kRpNone;
    rp_block_best(row, s, s_row, s_score);
    if (threadIdx.x == 0) {
        slab[2 * (uint64_t)blockIdx.x] = row;
        slab[2 * (uint64_t)blockIdx.x + 1] = row == kRpNone ? 0xFFF0000000000000ull : (uint64_t)__double_as_longlong(s);
    }
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rm_pick_kernel(const uint64_t *__restrict__ rows, int W, int n,
                                                             const uint64_t *__restrict__ slab, uint64_t n_blocks,
                                                             double shrink, int fresh, double *__restrict__ weights,
                                                             uint32_t *__restrict__ cover,
                                                             uint32_t *__restrict__ row_count,
                                                             uint64_t *__restrict__ state, uint32_t *__restrict__ picks,
                                                             uint32_t round, double *__restrict__ delta,
                                                             uint64_t *__restrict__ pick_word,
                                                             double *__restrict__ sum_word) {
#pragma clang fp contract(off)
    RP_LDS;
    double *s_w = reinterpret_cast<double *>(rp_lds);   // [64 * W]
    double *s_part = s_w + (size_t)64 * W;              // [64]
    uint64_t *s_row = reinterpret_cast<uint64_t *>(s_part + 64);
    double *s_score = reinterpret_cast<double *>(s_row + kRpThreads / 64);
    double &s_f = s_score[kRpThreads / 64];
    uint64_t &s_pick = reinterpret_cast<uint64_t *>(s_score)[kRpThreads / 64 + 1];
    uint64_t row;
    double score;
    rp_slab_best(slab, n_blocks, row, score, s_row, s_score);
    if (threadIdx.x == 0) {
        s_pick = row;
        *pick_word = row;
        if (picks) picks[round] = row == kRpNone ? kRpNoRow : (uint32_t)row;   // rows < cap < 2^32 - 1
        if (row != kRpNone) {
            row_count[row] += 1u;
            state[1] += 1ull;
        }
    }
    __syncthreads();
    const uint64_t p = s_pick;
    if (p == kRpNone) return;   // the whole workgroup: an empty table changes nothing else
    const uint64_t *prow = rows + p * W;
    for (int i = threadIdx.x; i < 64 * W; i += kRpThreads) {
        double v = 0.0, d = 0.0;
        if (i < n) {
            v = weights[i];
            if ((prow[i >> 6] >> (i & 63)) & 1) {
                const double shrunk = v * shrink;   // rounded before the subtract: contraction is off
                d = v - shrunk;
                v = shrunk;
                cover[i] += 1u;
                if (!fresh) weights[i] = v;
            }
        }
        s_w[i] = v;
        delta[i] = d;
    }
    if (!fresh) return;
    __syncthreads();
    const double s = rm_lane_sum(s_w, s_part, W);
    if (threadIdx.x == 0) s_f = (double)n / s;
    __syncthreads();
    const double f = s_f;
    for (int i = threadIdx.x; i < n; i += kRpThreads) {
        const double v = s_w[i] * f;
        s_w[i] = v;
        weights[i] = v;
    }
    __syncthreads();
    const double s2 = rm_lane_sum(s_w, s_part, W);
    if (threadIdx.x == 0) *sum_word = s2;
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rm_update_kernel(const uint64_t *__restrict__ rows,
                                                               const unsigned long long *__restrict__ d_len,
                                                               uint64_t cap, int W, const double *__restrict__ delta,
                                                               const uint64_t *__restrict__ pick_word,
                                                               double *__restrict__ scores, uint64_t *__restrict__ slab) {
#pragma clang fp contract(off)
    RP_LDS;
    const int Wp = (W + 1) & ~1;
    double *s_d = reinterpret_cast<double *>(rp_lds);                                  // [64 * W]
    uint64_t *s_p = reinterpret_cast<uint64_t *>(rp_lds + (size_t)64 * W * 8);         // [Wp]
    uint64_t *s_tiles = s_p + Wp;                                                      // [kRpThreads][kRpSegStride]
    uint64_t *s_row = reinterpret_cast<uint64_t *>(reinterpret_cast<unsigned char *>(s_tiles) + rp_tiles_lds());
    double *s_score = reinterpret_cast<double *>(s_row + kRpThreads / 64);
    const uint64_t len = min((uint64_t)*d_len, cap);
    const uint64_t row0 = (uint64_t)blockIdx.x * kRpTile;
    const uint64_t p = *pick_word;
    if (row0 >= len || p >= len) {   // the whole workgroup; p >= len only for an empty table (kRpNone)
        if (threadIdx.x == 0) {
            slab[2 * (uint64_t)blockIdx.x] = kRpNone;
            slab[2 * (uint64_t)blockIdx.x + 1] = 0xFFF0000000000000ull;
        }
        return;
    }
    for (int i = threadIdx.x; i < 64 * W; i += kRpThreads) s_d[i] = delta[i];
    for (int i = threadIdx.x; i < W; i += kRpThreads) s_p[i] = rows[p * W + i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *tile = s_tiles + (size_t)wave * 64 * kRpSegStride;
    const uint64_t wave_row0 = row0 + (uint64_t)wave * 64, my = wave_row0 + lane;
    const uint64_t *mine = tile + lane * kRpSegStride;
    __syncthreads();   // delta and row p
    // A wave stages its own 64 rows and reads only its own tile, so what orders the staging against the walk
    // is the wave's program order (rm_wave_sync), not a workgroup barrier: the four waves run apart.  Staging
    // takes 4 rows x kRpSeg words per instruction, lane = (row & 3, word) -- 128-byte runs, no division --,
    // and the next pass's words are loaded into registers before this pass's are walked.
    const int sr = lane >> 4, sw = lane & (kRpSeg - 1);
    uint64_t *put = tile + sr * kRpSegStride + sw;
    const uint64_t *get = rows + (wave_row0 + sr) * W + sw;
    auto touched = [&](int c0) {   // the first pass at or after c0 in which row p holds somebody
        for (; c0 < W; c0 += kRpSeg) {
            uint64_t any = 0;
            for (int w = c0; w < min(c0 + kRpSeg, W); ++w) any |= s_p[w];
            if (any) break;
        }
        return c0;
    };
    uint64_t buf[64 / 4];
    auto load = [&](int c0) {
#pragma unroll
        for (int it = 0; it < 64 / 4; ++it)
            buf[it] = (c0 + sw < W && wave_row0 + sr + 4 * it < len) ? get[(size_t)4 * it * W + c0] : 0ull;
    };
    double t = 0.0;
    int c0 = touched(0);
    if (c0 < W) load(c0);
    while (c0 < W) {
#pragma unroll
        for (int it = 0; it < 64 / 4; ++it) put[4 * it * kRpSegStride] = buf[it];
        rm_wave_sync();   // the staged words
        const int next = touched(c0 + kRpSeg);
        if (next < W) load(next);
        const int C = min(kRpSeg, W - c0);
        for (int w = 0; w < C; ++w) {
            const uint64_t pw = s_p[c0 + w];
            if (!pw) continue;   // the same for every lane
            uint64_t x = mine[w] & pw;
            const double *db = s_d + 64 * (c0 + w);
            while (x) {
                t = t + db[__ffsll((unsigned long long)x) - 1];
                x &= x - 1;
            }
        }
        rm_wave_sync();   // before the next pass overwrites the tile
        c0 = next;
    }
    const bool valid = my < len;
    double s = rp_minus_inf();
    if (valid) {
        s = scores[my] - t;
        scores[my] = s;
    }
    uint64_t row = valid ? my : kRpNone;
    rp_block_best(row, s, s_row, s_score);
    if (threadIdx.x == 0) {
        slab[2 * (uint64_t)blockIdx.x] = row;
        slab[2 * (uint64_t)blockIdx.x + 1] = (uint64_t)__double_as_longlong(s);
    }
}

template <int kLate = 0>
__global__ __launch_bounds__(kRpThreads) void rm_bound_kernel(const uint64_t *__restrict__ slab, uint64_t n_blocks,
                                                              const double *__restrict__ sum_word, int start,
                                                              uint64_t *__restrict__ state) {
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
            state[2] = kRpNone;
            state[3] = 0x7FF0000000000000ull;
        }
        return;
    }
    const double u = score / *sum_word;
    state[2] = row;
    state[3] = (uint64_t)__double_as_longlong(u);
    if (start || u < __longlong_as_double((long long)state[0])) state[0] = (uint64_t)__double_as_longlong(u);
}
