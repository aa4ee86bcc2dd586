// draw_lane.inc -- the batch LEGACY draw kernel (included by csa_legacy.hip inside its anonymous
// namespace; uses DrawArgs, select_bit, fmix_a/b, partner, raise_status and the outcome enum
// defined there).
//
// Same algorithm and bit-exact output as the reference in Philox verification mode
// (legacy.py:47-200, analysis.py:141-159), with TWO lanes per panel: a wavefront draws 32 panels at
// once and the only per-step cross-lane traffic is one DPP exchange inside each lane pair.  A lane
// holds its half of the panel's state in registers -- need = min - selected and remaining for
// FN / 2 features (FN <= 32) and WN / 2 words of the remaining pool (WN <= 32) -- so every
// per-feature / per-word loop is unrolled at compile time.  The picks are written as a list
// (picks16[panel][step], u16, rows of kpad = k rounded up to 8): each pair gathers eight picks in
// registers (four per lane) and stores them as one 16-byte chunk, so an accepted attempt leaves
// exactly its k picks there and no register copy of the picked or cascaded set is needed;
// picks_pack_kernel then builds the packed panel and its 128-bit hash.
//   * per-feature state: a feature with min = max = 0 ("dead": never a candidate, never full,
//     never failing -- exactly its role in legacy.py:124-157) is removed (zero bitmask row, no
//     person-mask bit, need = remaining = 0).  max = 0 < min instances use draw_kernel.
//   * find_max_ratio_cat (legacy.py:124-157): strict cross-multiplied argmax from the reference's
//     -100/1 sentinel with no explicit candidate test -- with every live remaining >= 0, (a)
//     remaining = 0 and need > 0 is the step's own SelectionError (legacy.py:132-137), (b)
//     remaining = 0 and need <= 0 never beats the strict comparison, (c) need <= -100 * remaining
//     never beats the sentinel, so the comparison against the sentinel start alone reproduces
//     legacy.py:138-149.  The FAIL test `remaining < min - selected` is read off the maximum
//     (ratio > 1, or need > 0 = remaining).
//   * holder scan (legacy.py:186-197): the second lane keeps the pool MIRRORED -- its words in
//     reversed order and each word bit-reversed (register j bit b = agent 64 WN - 1 - (64 j + b)) --
//     and looks for the (remaining[f*] - r + 1)-th holder counted from the last agent, which in its
//     own order is a plain scan from the start; so each lane finds its candidate in ONE pass over
//     its own words (no exchange of holder counts): it keeps the last word whose preceding holder
//     count is < r, then select_bit inside it, and the agent is off + sgn (64 word + bit) with
//     per-lane constants (0, +1) / (64 WN - 1, -1).
//   * delete_person (legacy.py:103-120): the picked person's feature mask (LDS) decrements need
//     and remaining; "selected == max" is a zero test of bit-sliced max - selected planes.
//   * delete_all_in_cat (legacy.py:47-62), bulk form: the cascading pairs of a step (up to
//     kLaneSlots per round) stage D = remaining & OR(rows of their full features) in per-wave LDS
//     slots; the 64 lanes then count popcount(D & featmask[g]) for every feature g (lane =
//     feature, half of the words) and each owner subtracts its row of decrements.
//   * post-pick SelectionErrors are deferred: remaining == 0 and selected < min inside the deletes
//     (legacy.py:55, 73) and the emptied pool (legacy.py:198-199) test exactly the next step's
//     start state, where the FAIL test and the no-candidate branch raise the same restart; after
//     the last pick the first becomes a min-quota rejection, also a restart.  Panels and attempt
//     counts are unchanged (every parity test, including the restart-heavy goldens).
//   * attempts start only on iterations it = 0 mod 8, so every running panel is at a step
//     s = it mod 8; every 8th iteration lane 0 of each pair computes the Philox block of steps
//     s..s+3 (block s/4, oracle/philox.py) and lane 1 that of steps s+4..s+7, the whole wave in
//     lockstep, and each step takes its word from the lane holding it (one DPP move); a panel
//     whose attempt ends waits at most 7 iterations for its next attempt.
// Built for 16 < F <= 32 (u32 person masks; F <= 16 takes draw_solo_kernel), W <= 32 and no
// max = 0 < min feature (draw_kernel covers the rest).

constexpr int kLaneThreads = 256;
constexpr int kLaneSlots = 8;  // cascading pairs per cooperative round (~1.8 cascades per step and wave at sf_e)

// hh: the household form, which keeps the address ring behind the cascade decrements
__host__ __device__ inline size_t lane_lds_bytes(int FN, int WN, int n, bool hh = false) {
    const size_t LS = (size_t)WN + 1;
    const size_t draw = (size_t)2 * FN * LS * 8 + 64                  // feature rows + mirrored rows (+ skew)
                        + (size_t)((n + 3) & ~3) * 4                  // person feature masks
                        + (size_t)4 * FN * 4                          // need0, rem0, mnx, pad
                        + (size_t)2 * WN * 8                          // attempt-start pool (+ mirrored)
                        + (size_t)(kLaneThreads / 64) * kLaneSlots * WN * 8   // cascade slots
                        + (size_t)(kLaneThreads / 64) * kLaneSlots * FN * 4   // cascade decrements
                        + (hh ? (size_t)((n + 3) & ~3) * 2 : 0);              // address ring (u16)
    // the fused pack reuses the space as a (panels of the workgroup) x (2 W + 1) u32 tile
    const size_t pack = (size_t)(kLaneThreads / 2) * (2 * (size_t)WN + 1) * 4;
    return draw > pack ? draw : pack;
}

// philox4x32_10 with the round keys recomputed in place: the compiler would otherwise hoist the
// 20 round keys of the loop-invariant seed into SGPRs and spill them to VGPR lanes
__device__ __forceinline__ void philox_lane(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0,
                                            uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        asm volatile("" : "+s"(k0), "+s"(k1));
        // one v_mad_u64_u32 per product (hi and lo words together), not a mul_hi + mul_lo pair
        const uint64_t p0 = (uint64_t)c0 * 0xD2511F53u, p1 = (uint64_t)c2 * 0xCD9E8D57u;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
    }
}

// acc + popcount(x) as ONE v_bcnt_u32_b32 (the compiler otherwise counts both halves of a
// 64-bit word from zero and adds them with a v_add3: three instructions per word)
__device__ __forceinline__ int bcnt_acc(uint32_t x, int acc) {
    int r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}

// Per-feature state packed in one 32-bit word: need = min - selected (signed, low half) and
// remaining (high half); |need|, remaining < 2^15 (n <= 16384).  Viewed as a short2 vector the
// cross-multiplied comparison compiles to two v_mul_i32_i24_sdwa with half-word selects, and the
// delete_person decrement of both halves to one packed 16-bit subtract.
typedef short short2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ short2_t as_s2(int v) { return __builtin_bit_cast(short2_t, v); }
__device__ __forceinline__ int as_i(short2_t v) { return __builtin_bit_cast(int, v); }
__device__ __forceinline__ int kneed(int key) { return (int)as_s2(key).x; }
__device__ __forceinline__ int krem(int key) { return (int)as_s2(key).y; }
__device__ __forceinline__ int kpack(int need, int rem) { return (int)(((uint32_t)rem << 16) | ((uint32_t)need & 0xFFFFu)); }
// key beats best under the reference's strict '>' on need/rem (legacy.py:145)
__device__ __forceinline__ bool kbeats(int key, int best) {
    const short2_t a = as_s2(key), b = as_s2(best);
    return (int)a.x * (int)b.y > (int)b.x * (int)a.y;
}

#ifndef CSA_LANE_OCC
#define CSA_LANE_OCC 4
#endif

// K8 (template parameter of the register kernels): the keys carry their feature index, so the argmax
// selects ONE register per feature (the key) instead of two (key and index).  Layout: remaining in
// the high half, need = min - selected as a signed byte in bits 0-7, and the index in bits 8-15
// stored as idx + 1 - [need < 0]: the packed 16-bit decrement of delete_person borrows from the index
// byte exactly once, when need crosses 0 -> -1 (need only decreases), so idx + 1 = byte 1 + [need < 0]
// holds throughout and never wraps (one bfe of the sign bit plus one add reading byte 1; the users
// fold the + 1 into their row base pointer).  The products read the need byte and the remaining half through SDWA
// selects, as the 16-bit form does.  Taken when every need stays in [-127, 127] (csa_instance::need8;
// sf_e, example_large_200), else the 16-bit keys (K8 = false) -- sf_e 270.0 -> 273.9 M panels/s.
typedef signed char schar4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int k8need(int key) { return (int)__builtin_bit_cast(schar4_t, key).x; }
__device__ __forceinline__ int k8rem(int key) { return (int)as_s2(key).y; }
__host__ __device__ inline int k8pack(int need, int rem, int idx) {
    return (int)(((uint32_t)rem << 16) | ((uint32_t)(idx + 1 - (need < 0)) & 0xFFu) << 8 | ((uint32_t)need & 0xFFu));
}
// idx + 1 (see above)
__device__ __forceinline__ int k8idx1(int key) { return (int)((((uint32_t)key >> 8) & 0xFFu) + (((uint32_t)key >> 7) & 1u)); }
// the argmax start value: need -100, remaining 1 (legacy.py:125); K8: index 0 (byte 1 = 0 + 1 - [need < 0])
template <bool K8>
constexpr int kDrawSentinel = K8 ? (1 << 16) | 0x009C : (1 << 16) | 0xFF9C;
__device__ __forceinline__ bool k8beats(int key, int best) {
    return k8need(key) * k8rem(best) > k8need(best) * k8rem(key);
}

// CSA_LANE_STAMPS (diagnostic builds only, tools/lane_stamps.py): per-wave s_memtime totals of
// four segments of the step loop, taken at wave-uniform points only (a stamp in divergent code
// would turn the accumulators into per-lane registers), summed into g_lane_stamps
#ifdef CSA_LANE_STAMPS
__device__ unsigned long long g_lane_stamps[24];
#define LANE_STAMP(k)                                              \
    do {                                                           \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();          \
        st_acc[k] += t_ - st_prev;                                 \
        st_prev = t_;                                              \
    } while (0)
// region markers (an asm comment in the .s, tools/valu_budget.py) and per-wave execution counters of
// the regions: the dynamic VALU mix = each region's static VALU x how often a wave runs it.  A region
// counts once per pass of the wave with any lane satisfying `cond`: the first active lane adds to the
// wave's LDS counter, so regions inside lane-divergent branches are counted whichever lanes run them
// (a per-lane register counter flushed from lane 0 missed every pass lane 0 sat out -- ADVICE r04)
#define LANE_REGION(name, k, cond)                                                                \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0); /* the scheduler moves nothing across a marker */      \
        asm volatile(";@region " #name);                                                          \
        const uint64_t b_ = __ballot(cond);                                                       \
        /* branch-free (every active lane adds, all but one add 0): no new basic block, so the */ \
        /* compiler lays the regions out as in the production build */                           \
        atomicAdd(&st_cnt[k], (uint32_t)(b_ != 0ull &&                                            \
                                         (int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1)); \
    } while (0)
#else
#define LANE_STAMP(k) \
    do {              \
    } while (0)
#define LANE_REGION(name, k, cond) \
    do {                           \
    } while (0)
#endif

// The register kernels' attempt-start tables -- feature rows (the lane kernel: also mirrored), person
// masks, start keys, slack planes, start pool -- depend only on the instance and its start state, so the
// host builds them once per state (draw_image_build, csa_legacy.hip) as one image in exactly the LDS
// layout below, and a workgroup's prologue is a copy.  Offsets in 8-byte words from the start of the
// dynamic LDS; need0 is followed by rem0 and the 2 FN words of slack planes (FN int32 each).
struct DrawImage {
    int fm_rev, pm, need0, pres0, pres0_rev, words;  // fm at 0; fm_rev / pres0_rev: the lane kernel only
};
__host__ __device__ constexpr DrawImage draw_image_layout(bool lane, int FN, int WN, int n) {
    DrawImage L = {};
    L.fm_rev = FN * (WN + 1) + 8;
    L.pm = lane ? L.fm_rev + FN * (WN + 1) : FN * (WN + 1);
    L.need0 = L.pm + ((n + 3) & ~3) / 2;
    L.pres0 = L.need0 + 2 * FN;
    L.pres0_rev = L.pres0 + WN;
    L.words = L.pres0 + (lane ? 2 : 1) * WN;  // even: FN is a multiple of 8, WN even
    return L;
}
// image -> LDS, 16 bytes per thread and trip; the trips of a batch issue their loads before the
// first store (one memory round trip per batch), whole batches without a bounds test
__device__ __forceinline__ void load_draw_image(uint64_t *smem, const uint64_t *image, int n16) {
    constexpr int B = 4, T = 256;  // both register kernels run 256 threads
    const uint4 *src = reinterpret_cast<const uint4 *>(image) + threadIdx.x;
    uint4 *dst = reinterpret_cast<uint4 *>(smem) + threadIdx.x;
    int base = 0;
    for (; base + B * T <= n16; base += B * T) {
        uint4 v[B];
#pragma unroll
        for (int u = 0; u < B; ++u) v[u] = src[base + u * T];
#pragma unroll
        for (int u = 0; u < B; ++u) dst[base + u * T] = v[u];
    }
    // the last batch is partial: its loads clamp their index to the image (no test), its stores test
    const int left = n16 - base - (int)threadIdx.x;  // this thread's trips left: ceil(left / T) <= B
    const uint4 *img = reinterpret_cast<const uint4 *>(image);
    uint4 v[B];
#pragma unroll
    for (int u = 0; u < B; ++u) v[u] = img[min(base + u * T + (int)threadIdx.x, n16 - 1)];
#pragma unroll
    for (int u = 0; u < B; ++u)
        if (u * T < left) dst[base + u * T] = v[u];
    __syncthreads();
}

// Pick-list layout.  The fused pack (A.panels set) uses a chunked layout per workgroup of PPW panels:
// chunk c (CH picks, steps c CH .. c CH + CH - 1) of the workgroup's panel p sits at u16 offset
// ((wg nch + c) PPW + p) CH, nch = kpad / CH -- the lanes of a wave store their chunks of one step
// side by side, so whole 128-byte lines leave L2 (the row layout's 16-byte pieces of 224-byte rows
// went out as partial lines: 491 MB of WRITE for 224 MB of lists at sf_e).  Both register kernels
// launch one workgroup per PPW panels (not persistent), so wg = blockIdx.x and PPW CH = 1024:
// offset = (blockIdx.x nch + c) 1024 + 4 threadIdx.x (two lanes x 4 picks, or one lane x 4).  The
// split path (csa_draw_picks_async, picks_pack_kernel) keeps the row layout picks16[i kpad + step].

// The fused pack of a draw kernel's tail: panels [pb, pb + rows) (rows <= kPackRows; pb a multiple
// of kPackRows inside a workgroup of PPW panels) from their chunked pick lists to bitmasks + 128-bit
// hashes, through a rows x (2 W + 1) u32 LDS tile (odd stride).  Called by all 256 threads of the
// workgroup after its draw; the leading barrier also makes the workgroup's own pick-list stores
// visible to every wave.  The chunks are read coalesced (consecutive threads: consecutive panels
// of one chunk index), every thread issuing all of its loads before the first use (one memory round
// trip -- the tail holds the workgroup's slot, so its latency is draw occupancy lost), OR-ed in with
// ds_or_b32; the rows are stored coalesced and each panel hashed by two lanes, exactly as
// picks_pack_kernel does.
constexpr int kPackRows = 128;
template <int PPW, int CH>
__device__ __forceinline__ void pack_tile_rows(const DrawArgs &A, uint32_t *tile, uint64_t pb, int rows) {
    static_assert(CH == 4 || CH == 8, "8- or 16-byte chunks");
    using unit_t = typename std::conditional<CH == 8, uint4, uint2>::type;
    const int W = A.W, k = A.k, kpad = (k + 7) & ~7, nch = kpad / CH;
    __syncthreads();
    const int R = 2 * W + 1;
    for (int t = threadIdx.x; 4 * t < kPackRows * R; t += blockDim.x) {
        if (4 * t + 3 < kPackRows * R) *reinterpret_cast<uint4 *>(tile + 4 * t) = make_uint4(0u, 0u, 0u, 0u);
        else for (int u = 4 * t; u < kPackRows * R; ++u) tile[u] = 0u;
    }
    const uint64_t wg = pb / PPW;
    const int p0 = (int)(pb % PPW);
    // unit (c, r) of this tile: chunk c of the workgroup's panel p0 + r
    const unit_t *src = reinterpret_cast<const unit_t *>(A.picks16 + (wg * nch * PPW + p0) * CH);
    __syncthreads();
    // A thread keeps one row, r = thread mod kPackRows, and takes the chunks c = thread / kPackRows + kRowSets u:
    // c is the same for a whole wave (kPackRows is a multiple of 64), so the tests on it are scalar
    // branches and only the row test masks lanes.  A chunk below the k-th pick ORs its CH picks
    // unconditionally; only the chunks that hold padding picks (steps >= k, stored as 0) test each pick.
    constexpr int kChunks = 8, kRowSets = kLaneThreads / kPackRows;
    static_assert(kPackRows % 64 == 0 && kLaneThreads % kPackRows == 0, "a wave's threads share their chunk index");
    const int r = (int)(threadIdx.x & (kPackRows - 1));
    const int cfirst = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kPackRows));
    if (r < rows) {
        uint32_t *trow = tile + r * R;
        const unit_t *srow = src + r;
        for (int c0 = cfirst; c0 < nch; c0 += kRowSets * kChunks) {
            unit_t v[kChunks];
#pragma unroll
            for (int u = 0; u < kChunks; ++u) {
                const int c = c0 + kRowSets * u;
                if (c < nch) v[u] = srow[(uint64_t)c * PPW];
            }
#pragma unroll
            for (int u = 0; u < kChunks; ++u) {
                const int c = c0 + kRowSets * u;
                if (c < nch) {
                    uint32_t w4[4];
                    if constexpr (CH == 8) {
                        w4[0] = v[u].x; w4[1] = v[u].y; w4[2] = v[u].z; w4[3] = v[u].w;
                    } else {
                        w4[0] = v[u].x; w4[1] = v[u].y; w4[2] = w4[3] = 0u;
                    }
                    if ((c + 1) * CH <= k) {
#pragma unroll
                        for (int h = 0; h < CH; ++h) {
                            const uint32_t q = (h & 1) ? w4[h >> 1] >> 16 : w4[h >> 1] & 0xFFFFu;
                            atomicOr(&trow[q >> 5], 1u << (q & 31));
                        }
                    } else {
#pragma unroll
                        for (int h = 0; h < CH; ++h) {
                            if (c * CH + h < k) {
                                const uint32_t q = (h & 1) ? w4[h >> 1] >> 16 : w4[h >> 1] & 0xFFFFu;
                                atomicOr(&trow[q >> 5], 1u << (q & 31));
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    // rows stored coalesced: element t = r W + w for t = thread, thread + 256, ...; the row, the word and the
    // tile address are carried from trip to trip (256 = dq W + dm, and a row's end adds R - 2 W = 1)
    uint64_t *dst = A.panels + pb * (uint64_t)W;
    {
        const int nt = rows * W, dq = kLaneThreads / W, dm = kLaneThreads - dq * W, step = dq * R + 2 * dm;
        int t = (int)threadIdx.x;
        // thread / W by a float reciprocal: exact for thread < 256, W <= 32 (t + 0.5 is >= 0.5 / W from an integer multiple)
        const int r0 = (int)(((float)t + 0.5f) * (1.0f / (float)W));
        int w = t - r0 * W;
        const uint32_t *tp = tile + r0 * R + 2 * w;
        for (; t < nt; t += kLaneThreads) {
            dst[t] = (uint64_t)tp[0] | ((uint64_t)tp[1] << 32);
            w += dm;
            tp += step;
            if (w >= W) {
                w -= W;
                tp += 1;
            }
        }
    }
    if (A.hashes) {  // two lanes per panel (threads 2r, 2r + 1), the words alternating
        const int r = threadIdx.x >> 1, sub = threadIdx.x & 1;
        uint64_t h1 = 0, h2 = 0;
        if (r < rows)
            for (int w = sub; w < W; w += 2) {
                const uint64_t x = (uint64_t)tile[r * R + 2 * w] | ((uint64_t)tile[r * R + 2 * w + 1] << 32);
                h1 += fmix_a(x ^ ((uint64_t)w * 0x9E3779B97F4A7C15ull));
                h2 += fmix_b(x + ((uint64_t)w + 1) * 0xD6E8FEB86659FD93ull);
            }
        h1 += partner64<0>(h1);
        h2 += partner64<0>(h2);
        if (r < rows && sub == 0) {
            A.hashes[2 * (pb + r)] = h1;
            A.hashes[2 * (pb + r) + 1] = h2;
        }
    }
}

// csa_draw_xt_async (A.xt set): a fused pack's tile rows [pb, pb + rows) (pb a multiple of 64, rows <=
// kPackRows, the tile as pack_tile_rows left it) also leave as XT, the pair kernels' operand: one 64 x 64
// register transpose (wave_transpose64, 30 VALU) per 64-panel block and 64-person word, written as
// csa_transpose_count_async writes them (plane 0: panels 0-31 of the block, plane 1: 32-63; npad persons,
// the padding words zero).  Read-only on the tile: the next pack_tile_rows starts with a barrier.
// A wave takes the words w = wave, wave + NWAVES, ... of each block: the block and the word are
// wave-uniform, so the stores are a scalar base plus the lane, the tile read steps one LDS address, and
// a trip is the transpose plus that step.  The tile's rows past `rows` are zero (pack_tile_rows clears
// all kPackRows and fills `rows`), so a partly empty block needs no row test; the padding words
// (w >= W) are stored as zeros without a transpose.
template <int NWAVES>
__device__ __forceinline__ void emit_xt_rows(const DrawArgs &A, const uint32_t *tile, uint64_t pb, int rows, int lane,
                                             int wave) {
    const XtLane tc = xt_lane_consts(lane);
    const int W = A.W, R = 2 * W + 1, npad = A.npad, nwd = npad / 64, nb = (rows + 63) / 64;
    const int w0 = __builtin_amdgcn_readfirstlane(wave);
    for (int blk = 0; blk < nb; ++blk) {
        const uint32_t *trow = tile + (64 * blk + lane) * R + 2 * w0;
        // the block's two planes (wave-uniform) and this lane's byte offset in them, stepped per word
        char *xlo = reinterpret_cast<char *>(A.xt + 2 * (pb / 64 + blk) * (uint64_t)npad), *xhi = xlo + 4 * (size_t)npad;
        uint32_t off = 4u * (uint32_t)(64 * w0 + lane);
        int w = w0;
        for (; w < W; w += NWAVES, trow += 2 * NWAVES, off += 256u * NWAVES) {
            uint32_t lo = trow[0], hi = trow[1];
            wave_transpose64(lo, hi, tc);
            *reinterpret_cast<uint32_t *>(xlo + off) = lo;
            *reinterpret_cast<uint32_t *>(xhi + off) = hi;
        }
        for (; w < nwd; w += NWAVES, off += 256u * NWAVES) {
            *reinterpret_cast<uint32_t *>(xlo + off) = 0u;
            *reinterpret_cast<uint32_t *>(xhi + off) = 0u;
        }
    }
}

// FN: features (padded, <= 32); WN: pool words (padded, <= 32, even per lane); SK: kept in the
// signature for the launcher (the holder scan reads all WN / 2 row words in one round trip); NP: slack
// bit planes kept (the instance's largest max - selected < 2^NP, csa_instance::max_slack)
// The two entry points share one function body, draw_lane_body.inc, compiled under each with
// CSA_DRAW_HH = 0 / 1 (HH in the body).  HH: the household form, as draw_solo_hh_kernel's (draw_solo.inc):
// the two lanes of a pair walk the pick's address ring together; the lane that holds a mate's word (the
// second lane: mirrored) drops its bit, and both take the mate's features off their remaining counts.
template <int FN, int WN, int SK, int NP, bool K8>
__global__ __launch_bounds__(kLaneThreads, CSA_LANE_OCC) void draw_lane_kernel(DrawArgs A)
#define CSA_DRAW_HH 0
#include "draw_lane_body.inc"
#undef CSA_DRAW_HH

// the household form (csa_instance_set_address_route CSA_ADDRESS_BATCH): all 8 slack planes
template <int FN, int WN, int SK, bool K8>
__global__ __launch_bounds__(kLaneThreads, CSA_LANE_OCC) void draw_lane_hh_kernel(DrawArgs A)
#define CSA_DRAW_HH 1
#include "draw_lane_body.inc"
#undef CSA_DRAW_HH

// picks16 (n_panels x kpad, pick order, kpad = k rounded up to 8) -> packed panels (n_panels x W,
// agent p = bit p & 63 of word p >> 6) + their 128-bit hashes (the key of the distinct-panel
// count).  One wave per PK panels: the wave's PK rows of picks are read coalesced (u32 = two
// picks) and OR-ed into a PK-row LDS tile (ds_or_b32, odd row stride of 2W + 1 u32), whose rows
// are then stored coalesced and hashed by 64 / PK lanes each.  PK shrinks with W so that a wave's
// tile stays near 8 KB (occupancy: n = 8192 takes PK = 4).  HBM-bound: 2 kpad B read + 8W + 16 B
// written per panel.
template <int PK>
__global__ __launch_bounds__(256) void picks_pack_kernel(const uint16_t *__restrict__ picks, uint64_t S, int k,
                                                         int W, uint64_t *__restrict__ panels,
                                                         uint64_t *__restrict__ hashes) {
    constexpr int LPP = 64 / PK;  // lanes per panel in the hash
    extern __shared__ uint32_t ptile_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const int R = 2 * W + 1;
    uint32_t *tile = ptile_all + wave * PK * R;
    const uint64_t i0 = ((uint64_t)blockIdx.x * nwv + wave) * PK;
    const int rows = i0 < S ? (int)min<uint64_t>(PK, S - i0) : 0;
    for (int t = lane; t < PK * R; t += 64) tile[t] = 0u;
    __syncthreads();
    const int kpad = (k + 7) & ~7;
    const int nu = rows * kpad;  // this wave's rows, contiguous from picks[i0 * kpad]
    const uint32_t *src = reinterpret_cast<const uint32_t *>(picks + i0 * (uint64_t)kpad);  // 16 B aligned
    const float rk = 1.0f / (float)kpad;
    for (int e = lane; 2 * e < nu; e += 64) {
        const uint32_t v = src[e];  // kpad even: both halves inside the wave's rows
        // row = q / kpad: float reciprocal, exact for q < 64 kpad, kpad <= 16384 (error < 2^-17 < 0.5/kpad)
        const int r = min(rows - 1, (int)(((float)(2 * e) + 0.5f) * rk));
        const int c = 2 * e - r * kpad;  // step of the low half (c + 1: the high half, same row)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (c + h < k) {
                const uint32_t p = h ? v >> 16 : v & 0xFFFFu;
                atomicOr(&tile[r * R + (p >> 5)], 1u << (p & 31));
            }
        }
    }
    __syncthreads();
    uint64_t *dst = panels + i0 * (uint64_t)W;
    const float rw = 1.0f / (float)W;
    for (int t = lane; t < rows * W; t += 64) {
        const int r = min(rows - 1, (int)(((float)t + 0.5f) * rw)), w = t - r * W;
        dst[t] = (uint64_t)tile[r * R + 2 * w] | ((uint64_t)tile[r * R + 2 * w + 1] << 32);
    }
    if (hashes) {
        const int r = lane / LPP, sub = lane - r * LPP;
        uint64_t h1 = 0, h2 = 0;
        if (r < rows)
            for (int w = sub; w < W; w += LPP) {
                const uint64_t x = (uint64_t)tile[r * R + 2 * w] | ((uint64_t)tile[r * R + 2 * w + 1] << 32);
                h1 += fmix_a(x ^ ((uint64_t)w * 0x9E3779B97F4A7C15ull));
                h2 += fmix_b(x + ((uint64_t)w + 1) * 0xD6E8FEB86659FD93ull);
            }
        if constexpr (LPP >= 2) { h1 += partner64<0>(h1); h2 += partner64<0>(h2); }
        if constexpr (LPP >= 4) { h1 += partner64<1>(h1); h2 += partner64<1>(h2); }
        if constexpr (LPP >= 8) { h1 += partner64<2>(h1); h2 += partner64<2>(h2); }
        if constexpr (LPP >= 16) { h1 += partner64<3>(h1); h2 += partner64<3>(h2); }
        if (r < rows && sub == 0) {
            hashes[2 * (i0 + r)] = h1;
            hashes[2 * (i0 + r) + 1] = h2;
        }
    }
}
