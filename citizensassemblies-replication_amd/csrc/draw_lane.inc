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

__host__ __device__ inline size_t lane_lds_bytes(int FN, int WN, int n) {
    const size_t LS = (size_t)WN + 1;
    const size_t draw = (size_t)2 * FN * LS * 8 + 64                  // feature rows + mirrored rows (+ skew)
                        + (size_t)((n + 3) & ~3) * 4                  // person feature masks
                        + (size_t)4 * FN * 4                          // need0, rem0, mnx, pad
                        + (size_t)2 * WN * 8                          // attempt-start pool (+ mirrored)
                        + (size_t)(kLaneThreads / 64) * kLaneSlots * WN * 8   // cascade slots
                        + (size_t)(kLaneThreads / 64) * kLaneSlots * FN * 4;  // cascade decrements
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
template <int FN, int WN, int SK, int NP, bool K8>
__global__ __launch_bounds__(kLaneThreads, CSA_LANE_OCC) void draw_lane_kernel(DrawArgs A) {
    constexpr int G = 2;
    constexpr int LS = WN + 1;        // odd row stride: lanes reading different rows hit different banks
    constexpr int WS = (WN + 1) / 2;  // words per half-wave in the cooperative cascade
    constexpr int FPL = FN / G, WPL = WN / G;
    // built for F > 16 only (FN = 32: F <= 16 takes draw_solo_kernel), so a lane holds 16 features and
    // the full test is always the bit-sliced slack planes
    static_assert(FN == 32 && WN <= 32 && (WN % 2) == 0 && SK >= 1 && NP >= 1 && NP <= 8, "lane draw layout");
    extern __shared__ uint64_t smem[];
    const int n = A.n, k = A.k;
    const DrawImage L = draw_image_layout(true, FN, WN, n);
    uint64_t *fm = smem;
    // row f word t = fm row f word WN-1-t, bit-reversed (the second lane's mirrored order).  Skewed by 8 words: FN * LS words is
    // a multiple of 32 dwords, so without it the two lanes of a pair read the same bank pair of the
    // 32 a ds_read2_b64 uses (a 2-way conflict on every scan read); 8 words put them 16 banks apart
    uint64_t *fm_rev = fm + L.fm_rev;
    uint32_t *pm = reinterpret_cast<uint32_t *>(fm + L.pm);
    int32_t *need0_s = reinterpret_cast<int32_t *>(fm + L.need0);
    int32_t *rem0_s = need0_s + FN, *mnx_s = need0_s + 2 * FN;  // mnx_s: the slack bit planes
    uint64_t *pres0_s = fm + L.pres0;
    uint64_t *pres0_rev = fm + L.pres0_rev;  // word t = pool word WN-1-t, bit-reversed
    uint64_t *slot_all = fm + L.words;
    int32_t *dec_all = reinterpret_cast<int32_t *>(slot_all + (kLaneThreads / 64) * kLaneSlots * WN);

    // everything below slot_all is the instance's image (draw_image_build): dead features (min = max = 0)
    // removed from the rows and the person masks, the start keys packed, the slack planes sliced
    // (mnx_s[8 glane + i] bit j = bit i of the slack of feature glane * FPL + j; dead and padding
    // features all ones, never picked, so never 0), the start pool also mirrored
    load_draw_image(smem, A.image, L.words / 2);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int glane = lane & 1, gbase = lane & ~1;
    const int fbase = glane * FPL;
    const uint64_t *fmx = glane ? fm_rev : fm;  // rows in this lane's order
    // agent of position m = 64 word + bit in this lane's order: poff + psgn m
    const int poff = glane ? 64 * WN - 1 : 0, psgn = glane ? -1 : 1;
    uint64_t *slots = slot_all + (size_t)wave * kLaneSlots * WN;
    int32_t *decs = dec_all + wave * kLaneSlots * FN;
    const uint32_t key0 = (uint32_t)A.seed, key1 = (uint32_t)(A.seed >> 32);
    // wave-uniform (SGPRs): a VGPR copy would be spilled
    const uint64_t n_groups = (uint64_t)__builtin_amdgcn_readfirstlane(gridDim.x * (blockDim.x / G));
    const uint64_t *pres0_l = glane ? pres0_rev : pres0_s;
    uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / G) + (threadIdx.x / G);
    bool active = i < A.n_panels;
    if (active && __hip_atomic_load(&A.status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) active = false;
    bool started = false;
    uint32_t a = 0;
    int s = 0;
    int key[FPL];      // packed (need, remaining) per feature
    uint64_t rm[WPL];  // remaining pool, this lane's words in its scan order
    // picks of steps 8c + 4 glane .. 8c + 4 glane + 3 (u16 each, two per dword), stored per 8 steps
    uint32_t pacc_lo = 0u, pacc_hi = 0u;
    uint32_t sp[NP];       // slack bit planes of this lane's features (see mnx_s above)
#pragma unroll
    for (int q = 0; q < NP; ++q) sp[q] = 0u;
    const int kpad = (k + 7) & ~7;
#pragma unroll
    for (int j = 0; j < FPL; ++j) key[j] = 0;
#pragma unroll
    for (int j = 0; j < WPL; ++j) rm[j] = 0ull;
    uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;

#ifdef CSA_LANE_STAMPS
    uint64_t st_acc[4] = {0, 0, 0, 0};
    // loop, philox, step, pick, store, round, pass2, pass1, nocand, kcheck, ending
    __shared__ uint32_t st_cnt_all[kLaneThreads / 64][11];
    uint32_t *st_cnt = st_cnt_all[threadIdx.x >> 6];
    if ((threadIdx.x & 63) < 11) st_cnt[threadIdx.x & 63] = 0u;
    uint64_t st_prev = __builtin_amdgcn_s_memtime();
#endif
    for (uint32_t it = 0; __ballot(active) != 0ull; ++it) {
        LANE_REGION(loop, 0, true);
        // ---- attempt starts (legacy_find's fresh deepcopy, analysis.py:147-148) + Philox --------
        // The two lanes of a pair compute alternate Philox blocks: every 8th iteration lane 0 computes
        // block s/4 (steps s..s+3) and lane 1 block s/4 + 1 (steps s+4..s+7), and each step takes its
        // word from the lane that holds it (one DPP move) -- half the Philox VALU of both lanes
        // computing the same block every 4th iteration.  Attempts therefore start on iterations
        // it = 0 mod 8 (no wait at all when every panel takes one attempt, as at sf_e).
        if ((it & 7u) == 0u) {
            LANE_REGION(philox, 1, true);
            if (active && !started) {
#pragma unroll
                for (int j = 0; j < FPL; ++j)  // K8: packed with its index at kernel start
                    key[j] = K8 ? need0_s[fbase + j] : kpack(need0_s[fbase + j], rem0_s[fbase + j]);
#pragma unroll
                for (int q = 0; q < NP; ++q) sp[q] = (uint32_t)mnx_s[8 * glane + q];
#pragma unroll
                for (int j = 0; j < WPL; ++j) rm[j] = pres0_l[j];
                started = true;
                s = 0;
                pacc_lo = pacc_hi = 0u;
            }
            const uint64_t panel = A.panel_begin + i;
            x0 = ((uint32_t)s >> 2) + (uint32_t)glane;
            x1 = A.attempt_base + a;
            x2 = (uint32_t)panel;
            x3 = (uint32_t)(panel >> 32);
            philox_lane(x0, x1, x2, x3, key0, key1);
        }

        LANE_STAMP(0);  // attempt starts + Philox
        // ---- one step: find_max_ratio_cat + holder pick + delete_person -------------------------
        int outcome = kContinue;
        uint32_t fl = 0;  // the pick's features (this lane's share) that reached max
        LANE_REGION(step, 2, started);
        if (started) {
            constexpr int kSentinel = kDrawSentinel<K8>;
            int best, bi;
            if constexpr (K8) {
                // two independent chains (features [0, H) and [H, FPL)) merged at the end (chain A wins
                // ties: the first maximum); the key carries its index, so one select per feature
                constexpr int H = FPL / 2;
                int bA = kSentinel, bB = kSentinel;
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    const bool tA = k8beats(key[j], bA);
                    const bool tB = k8beats(key[H + j], bB);
                    bA = tA ? key[j] : bA;
                    bB = tB ? key[H + j] : bB;
                }
                best = k8beats(bB, bA) ? bB : bA;
                {  // the pair's DPP exchange: lane 0 holds the lower indices, so it wins ties
                    const int ob = partner<0>(best);
                    const int l = k8need(ob) * k8rem(best), r = k8need(best) * k8rem(ob);
                    best = l > r - glane ? ob : best;  // lane 1 also takes a tie (|products| < 2^23)
                }
                bi = k8idx1(best);  // index + 1: the row base below is one row early
            } else {
                // two independent chains (features [0, H) and [H, FPL)) merged at the end: each chain
                // is a serial mul -> compare -> select dependency, so interleaving two of them fills
                // the VALU-to-mask wait states of the other; the merge keeps chain A on ties (lower
                // indices), i.e. the first maximum, as the single strict-'>' chain
                // (chain-local indices: inline constants in the selects, no VGPR per feature index)
                constexpr int H = FPL / 2;
                int bA = kSentinel, iA = 0, bB = kSentinel, iB = H;
#pragma unroll
                for (int j = 0; j < H; ++j) {
                    const bool tA = kbeats(key[j], bA);
                    const bool tB = kbeats(key[H + j], bB);
                    bA = tA ? key[j] : bA;
                    iA = tA ? j : iA;
                    bB = tB ? key[H + j] : bB;
                    iB = tB ? H + j : iB;
                }
                const bool tm = kbeats(bB, bA);
                best = tm ? bB : bA;
                bi = fbase + (tm ? iB : iA);
                {  // the pair's DPP exchange (lowest feature index on ties)
                    const int ob = partner<0>(best), oi = partner<0>(bi);
                    const short2_t x = as_s2(ob), y = as_s2(best);
                    const int l = (int)x.x * (int)y.y, r = (int)y.x * (int)x.y;
                    const bool take = (l > r) | ((l == r) & (oi < bi));
                    best = take ? ob : best;
                    bi = take ? oi : bi;
                }
            }
            const int bn = K8 ? k8need(best) : kneed(best), bd = krem(best);
            if ((bd == 0) | (bn > bd)) {
                outcome = kFail;  // legacy.py:132-137
            } else if (best == kSentinel) {
                LANE_REGION(nocand, 8, true);
                bool ne = false;
#pragma unroll
                for (int j = 0; j < WPL; ++j) ne |= rm[j] != 0ull;
                // KeyError (legacy.py:188), or the previous step's deferred emptied-pool error
                outcome = (max((int)ne, partner<0>((int)ne)) || s == 0) ? kNoCandidate : kFail;
            } else {
                LANE_REGION(pick, 3, true);
                const int q = (int)(it & 3u);  // == s & 3 for every running pair
                const uint32_t mine_w = q == 0 ? x0 : (q == 1 ? x1 : (q == 2 ? x2 : x3));
                const uint32_t other_w = (uint32_t)partner<0>((int)mine_w);
                const uint32_t word = ((it >> 2) & 1u) == (uint32_t)glane ? mine_w : other_w;
                const int r = 1 + (int)__umulhi(word, (uint32_t)bd);  // randint(1, rem[f*]), legacy.py:149
                const uint64_t *row = (K8 ? fmx - LS : fmx) + bi * LS;
                // rank sought among this lane's words in its scan order
                const int rr = glane ? bd - r + 1 : r;
                uint64_t rw[WPL];  // every row read issued before the scan (one LDS round trip)
#pragma unroll
                for (int j = 0; j < WPL; ++j) rw[j] = row[j];
                // the scan runs over word PAIRS: the pair whose preceding holder count is < rr is
                // kept (both masked words, the count before it), then one compare picks the word
                // inside it.  Every pair forms its masked words and counts them for all lanes (the
                // count chain never waits on a predicate); the keep is four moves under the pair's
                // own lane predicate `acc < rr` -- v_mov_b32 for the count and the index, one
                // v_mov_b64 per masked word -- instead of six v_cndmask.  The scheduling barrier (no
                // instruction) keeps the body from being turned back into selects.
                // (rr >= 1 on both lanes, so the first pair is always taken: it initialises the kept
                // pair and the predicated keeps start at the second)
                // (`acc < rr` is monotone, and draw_solo_kernel nests the pairs under a narrowing
                // predicate, a lane leaving the scan at the first pair it does not take; here, with
                // seven pairs and one lane of each pair scanning to the end, the nested form put the
                // compare -> exec -> count chain in series and measured 1.1 % slower at sf_e:
                // DESIGN 4.1)
                int base = 0, wsp = 0;
                uint64_t ma = rm[0] & rw[0], mb = rm[1] & rw[1];
                int acc = bcnt_acc((uint32_t)(ma >> 32), bcnt_acc((uint32_t)ma, 0));
                acc = bcnt_acc((uint32_t)(mb >> 32), bcnt_acc((uint32_t)mb, acc));
#pragma unroll
                for (int j = 2; j < WPL; j += 2) {
                    const uint64_t m0 = rm[j] & rw[j], m1 = rm[j + 1] & rw[j + 1];
                    if constexpr (WN < 32) {
                        if (acc < rr) {
                            base = acc;
                            wsp = j;
                            ma = m0;
                            mb = m1;
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    } else {  // WN = 32 has no register to spare: the predicated form spills there
                        const bool tk = acc < rr;
                        base = tk ? acc : base;
                        wsp = tk ? j : wsp;
                        ma = tk ? m0 : ma;
                        mb = tk ? m1 : mb;
                    }
                    acc = bcnt_acc((uint32_t)(m0 >> 32), bcnt_acc((uint32_t)m0, acc));
                    acc = bcnt_acc((uint32_t)(m1 >> 32), bcnt_acc((uint32_t)m1, acc));
                }
                // exactly one lane of the pair holds the r-th holder: lane 0 iff r <= its count,
                // lane 1 iff bd - r + 1 <= its count (the two counts add up to bd)
                const bool hit = rr <= acc;
                const int c0 = __popcll(ma);
                const bool second = rr - base > c0;  // the holder is in the pair's second word
                const uint64_t ms = second ? mb : ma;
                const int ws = wsp + (int)second;
                const int kin = hit ? rr - base - (second ? c0 : 0) : 1;
                const int b = select_bit(ms, kin);
                const int pl = hit ? poff + psgn * (ws * 64 + b) : -1;
                const int p = max(pl, partner<0>(pl));
                const uint32_t hb = pm[p] >> fbase;
                {
#pragma unroll
                    for (int j = 0; j < FPL; ++j) {
                        const int hneg = (int)(hb << (31 - j)) >> 31;  // -has
                        key[j] = as_i(as_s2(key[j]) + (short2_t)(short)hneg);
                    }
                    // selected == max after this pick (legacy.py:113-114) <=> the feature's slack
                    // max - selected reaches 0: a bit-sliced decrement of the pick's features (two
                    // VALU per bit plane for all FPL features at once) and a zero test of the planes
                    // (~21 VALU instead of 2 per feature).  Only the pick's own features can have just
                    // become full (an earlier full feature has no holder left; no feature starts at max:
                    // csa_instance::sel_over_max routes those elsewhere).
                    uint32_t bw = hb & 0xFFFFu;
                    const uint32_t picked = bw;
                    uint32_t nz = 0u;
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const uint32_t t = sp[q];
                        sp[q] = t ^ bw;
                        nz |= sp[q];
                        if (q + 1 < NP) bw &= ~t;
                    }
                    fl = (picked & ~nz) << fbase;
                }
                LANE_REGION(update, 0, false);  // (runs with `pick`)
                // drop the pick from the register pool: the picked bit is set in rm[ws] (it was taken
                // from rm[ws] & row[ws]), so clearing it is subtracting it -- one 64-bit add of -(1 << b)
                // = ~0 << b.  Each lane forms the addends of a pair's two words once (the other word's
                // is 0) and each pair adds them under its own lane predicate (the hit lane whose kept
                // pair it is): a compare and two v_lshl_add_u64 per pair instead of a bfe + two
                // v_bitop3 per word.  The non-hit lane matches no pair and leaves its pool untouched.
                // The scheduling barrier (no instruction) keeps the body from being turned into
                // selects; unlike an empty asm it leaves the compiler free to drop the skip branch
                // around the two adds.
                {
                    const uint64_t nb = ~0ull << b;
                    const uint64_t dA = second ? 0ull : nb, dB = second ? nb : 0ull;
                    const int wh = hit ? wsp : -1;
#pragma unroll
                    for (int j = 0; j < WPL; j += 2) {
                        if (wh == j) {
                            rm[j] += dA;
                            rm[j + 1] += dB;
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
                // the pick of step s joins its 8-step chunk (lane 0: slots 0-3, lane 1: slots 4-7);
                // the pair stores the chunk as 16 contiguous bytes after its 8th step or the k-th.
                // (Round 1 OR-ed each pick's bit into the output row with a 64-bit atomic: MI355X
                // performs global atomics at the memory side, 3.7 GB of HBM writes per 10^6 sf_e
                // panels for 216 MB of panels; one 2-byte store per pick still wrote 1.46 GB, its
                // partial lines leaving L2 before the row was complete.)
                {
                    // slot = s & 7 = it & 7 for every running pair (attempts start on it = 0 mod 8), so
                    // the dword and the shift are wave-uniform: a scalar branch and one shift-or
                    // (a 64-bit shift by a per-lane amount and two selects before)
                    const int slot = __builtin_amdgcn_readfirstlane((int)(it & 7u));
                    const uint32_t pv = ((slot >> 2) == glane) ? (uint32_t)p : 0u;  // 0 <= p < 2^15
                    if (slot & 2) pacc_hi |= pv << (16 * (slot & 1));
                    else pacc_lo |= pv << (16 * (slot & 1));
                    LANE_REGION(store, 4, (slot == 7) | (s == k - 1));
                    if ((slot == 7) | (s == k - 1)) {
                        const uint64_t off = A.panels ? ((uint64_t)blockIdx.x * (kpad >> 3) + (uint64_t)(s >> 3)) * 1024 +
                                                            4 * threadIdx.x
                                                      : i * (uint64_t)kpad + (s & ~7) + 4 * glane;
                        *reinterpret_cast<uint64_t *>(A.picks16 + off) = ((uint64_t)pacc_hi << 32) | pacc_lo;
                        pacc_lo = pacc_hi = 0u;
                    }
                }
                LANE_REGION(update, 0, false);
                fl |= (uint32_t)partner<0>((int)fl);  // both lanes of the pair see all full features
            }
        }
        LANE_STAMP(1);  // the step: argmax, holder scan, select, decrements

        // ---- the k-th pick: check_min_cats (legacy.py:160-168, analysis.py:155-159) now, and no
        // cascade for a panel that passes -----------------------------------------------------------
        // After the last pick nothing reads the pool or remaining again, except the rejection
        // classifier below (need > 0 = remaining) of a pair with some need > 0.  A pair with every
        // need <= 0 is accepted whatever its cascade would leave (it cannot raise legacy.py:55, and
        // legacy.py:198-199 applies before the last step only), so its full features are dropped
        // here; an under-quota pair cascades as ever when the statistics are wanted.  The branch is
        // wave-uniform: an ordinary step pays the compare.
        const bool last = started & (outcome == kContinue) & (s == k - 1);
        if (__ballot(last) != 0ull) {
            LANE_REGION(kcheck, 9, true);
            bool u = false;
#pragma unroll
            for (int j = 0; j < FPL; ++j) u |= (K8 ? k8need(key[j]) : kneed(key[j])) > 0;
            const bool under = max((int)u, partner<0>((int)u)) != 0;
            if (last) {
                outcome = under ? kReject : kAccept;
                if (!(under && A.stats)) fl = 0u;
            }
        }

        // ---- delete_all_in_cat, wave-cooperative in rounds of kLaneSlots cascading pairs ---------
        uint64_t cb = __ballot(fl != 0u && glane == 0);
        LANE_REGION(cascade, 5, false);
        while (cb) {
            LANE_REGION(round, 5, true);
            uint64_t rb = cb;  // usually all of them fit one round
            if (__popcll(cb) > kLaneSlots) {
                rb = 0ull;
#pragma unroll
                for (int j = 0; j < kLaneSlots; ++j) {
                    const uint64_t low = cb & (~cb + 1ull);
                    rb |= low;
                    cb ^= low;
                }
            } else {
                cb = 0ull;
            }
            const bool mine = (rb >> gbase) & 1ull;
            // slot = set bits of rb below the pair's first lane (v_mbcnt counts the bits below this
            // lane; rb holds first lanes only, so the second lane subtracts its partner's bit)
            const int slot = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(rb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rb, 0u)) -
                             (int)(glane & (uint32_t)mine);
            uint64_t *srow = slots + (mine ? slot : 0) * WN + glane * WPL;
            if (mine) {
                // remaining &= ~OR(rows of the full features) (this lane's words; one v_bfi per
                // dword), and the slot receives the NEW pool: the counting pass below then yields
                // every feature's remaining count outright (popcount(pool & featmask[g]) is exactly
                // what the decrements by popcount(D & featmask[g]) would leave), so D itself is
                // never formed.  Usually one feature is full; further ones add their still-remaining
                // holders.  All row reads are issued before the first slot write (an interleaved
                // read/write sequence waits one LDS round trip per word).
                uint32_t bits = fl;
                const uint64_t *f0 = fmx + __builtin_ctz(bits) * LS;
                bits &= bits - 1u;
                uint64_t orr[WPL];
#pragma unroll
                for (int j = 0; j < WPL; ++j) orr[j] = f0[j];
                while (bits) {
                    const uint64_t *fr = fmx + __builtin_ctz(bits) * LS;
                    bits &= bits - 1u;
#pragma unroll
                    for (int j = 0; j < WPL; ++j) orr[j] |= fr[j];
                }
#pragma unroll
                for (int j = 0; j < WPL; ++j) {
                    rm[j] &= ~orr[j];
                    srow[j] = rm[j];
                }
            }
            // rem[g] = popcount(pool & featmask[g]): lane = (feature g, word half); slot words
            // WPL.. hold the second lane's words mirrored, paired with fm_rev
            const int g = lane & 31, half = lane >> 5;
            const int w0 = half * WS;
            const uint64_t *frow = (half ? fm_rev - WS : fm) + (g < FN ? g : 0) * LS;
            const int ns = __popcll(rb);
            // slots in pairs per pass over the feature row (half the row reads, two independent
            // chains); an odd last slot gets a one-slot pass (~1.8 cascading pairs per wave-step
            // at sf_e, so ns = 1 is the common round)
            auto count_pass = [&](int q0, auto two_c) {
                constexpr bool TWO = decltype(two_c)::value;
                if constexpr (TWO) LANE_REGION(pass2, 6, true);
                else LANE_REGION(pass1, 7, true);
                const uint64_t *d0 = slots + q0 * WN, *d1 = d0 + WN;
                int c0 = 0, c1 = 0;
                constexpr int CK = 2;  // words per batch of slot reads (larger batches: more VGPRs, no faster)
#pragma unroll
                for (int t0 = 0; t0 < WS; t0 += CK) {
                    uint64_t a0[CK], a1[CK];
#pragma unroll
                    for (int u = 0; u < CK; ++u) {
                        const int w = w0 + t0 + u;
                        const bool ok = t0 + u < WS;
                        a0[u] = ok ? d0[w] : 0ull;
                        a1[u] = (TWO && ok) ? d1[w] : 0ull;
                    }
#pragma unroll
                    for (int u = 0; u < CK; ++u) {
                        const int w = w0 + t0 + u;
                        if (t0 + u < WS) {
                            const uint64_t f = frow[w];
                            const uint64_t x0 = a0[u] & f;
                            c0 = bcnt_acc((uint32_t)(x0 >> 32), bcnt_acc((uint32_t)x0, c0));
                            if constexpr (TWO) {
                                const uint64_t x1 = a1[u] & f;
                                c1 = bcnt_acc((uint32_t)(x1 >> 32), bcnt_acc((uint32_t)x1, c1));
                            }
                        }
                    }
                }
                // + the other word half (lane +- 32): v_permlane32_swap, no LDS round trip
                const auto s0 = __builtin_amdgcn_permlane32_swap(c0, c0, false, false);
                c0 = s0[0] + s0[1];
                if constexpr (TWO) {
                    const auto s1 = __builtin_amdgcn_permlane32_swap(c1, c1, false, false);
                    c1 = s1[0] + s1[1];
                }
                if (lane < FN) {  // remaining is the key's high half
                    decs[q0 * FN + lane] = c0 << 16;
                    if constexpr (TWO) decs[(q0 + 1) * FN + lane] = c1 << 16;
                }
            };
            int q0 = 0;
            for (; q0 + 1 < ns; q0 += 2) count_pass(q0, std::true_type{});
            if (q0 < ns) count_pass(q0, std::false_type{});
            if (mine) {
                const int32_t *dv = decs + slot * FN + fbase;
#pragma unroll
                for (int j = 0; j < FPL; j += 4) {
                    const int4 v = *reinterpret_cast<const int4 *>(dv + j);
                    // remaining (high half) replaced by the recount; need (low half) kept
                    key[j] = (key[j] & 0xFFFF) | v.x;
                    key[j + 1] = (key[j + 1] & 0xFFFF) | v.y;
                    key[j + 2] = (key[j + 2] & 0xFFFF) | v.z;
                    key[j + 3] = (key[j + 3] & 0xFFFF) | v.w;
                }
            }
        }

        LANE_STAMP(2);  // cascades
        LANE_REGION(book, 0, false);
        // ---- bookkeeping: the k-th pick's min-quota check, restarts, accepted panels -------------
        if (started) {
            if (outcome == kContinue) ++s;  // (the k-th pick's outcome was set before the cascades)
            LANE_REGION(book, 0, false);
            if (outcome != kContinue) {
                LANE_REGION(ending, 10, true);
                const uint64_t panel = A.panel_begin + i;
                started = false;  // the next attempt / panel starts at the next iteration it = 0 mod 8
                s = 0;
                if (outcome == kNoCandidate) {
                    if (glane == 0) raise_status(A.status, CSA_E_NO_CANDIDATE, panel);
                    active = false;
                } else if (outcome != kAccept) {  // SelectionError restart / min-quota rejection
                    if (A.stats) {
                        // the deferred post-pick test: after the k-th pick a feature with remaining
                        // == 0 and selected < min is the reference's SelectionError (legacy.py:55,
                        // 73), raised before check_min_cats; the other restarts are rejections
                        int rj = outcome == kReject;
                        if (rj) {
                            bool dead = false;
#pragma unroll
                            for (int j = 0; j < FPL; ++j)
                                dead |= (K8 ? k8need(key[j]) : kneed(key[j])) > 0 && krem(key[j]) == 0;
                            rj = !max((int)dead, partner<0>((int)dead));
                        }
                        if (glane == 0) atomicAdd(A.stats + rj, 1ull);
                    }
                    if (++a >= A.max_attempts) {
                        if (glane == 0) raise_status(A.status, CSA_E_ATTEMPT_LIMIT, panel);
                        active = false;
                    }
                } else {  // picks16 already holds this attempt's k picks (its last chunk was stored at s = k-1)
                    if (A.attempts && glane == 0) A.attempts[i] = a + 1;
                    // no status poll here: a load in the loop would wait on vmcnt, i.e. on the
                    // wave's outstanding pick stores; after an error elsewhere this pair just
                    // finishes its panels
                    i += n_groups;
                    a = 0;
                    active = i < A.n_panels;
                }
            }
        }
        LANE_STAMP(3);  // bookkeeping + loop control
    }
    LANE_REGION(tail, 0, false);

    // ---- fused pack (A.panels set, csa_draw_async): this workgroup's panels -> bitmasks + hashes
    // The launch is not persistent, so the workgroup drew panels [128 b, 128 b + 128) and their
    // pick lists are in picks16 (written by its own waves).  After a workgroup barrier -- which
    // also makes those stores visible to every wave of the workgroup -- the LDS becomes a
    // 128 x (2 W + 1) u32 tile (odd stride): the pick lists are read coalesced and OR-ed in
    // (ds_or_b32), the rows stored coalesced, and each panel hashed by two lanes, exactly as
    // picks_pack_kernel does.  The pack's HBM traffic then overlaps other workgroups' VALU-bound
    // draws instead of running as a separate kernel after the whole draw.
    if (A.panels) {
        constexpr int PW = kLaneThreads / G;  // panels of the workgroup
        const uint64_t pb = (uint64_t)blockIdx.x * PW;
        const int rows = pb < A.n_panels ? (int)min<uint64_t>(PW, A.n_panels - pb) : 0;
        pack_tile_rows<kLaneThreads / 2, 8>(A, reinterpret_cast<uint32_t *>(smem), pb, rows);
        if (A.xt) emit_xt_rows<kLaneThreads / 64>(A, reinterpret_cast<const uint32_t *>(smem), pb, rows, lane, wave);
    }
#ifdef CSA_LANE_STAMPS
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) atomicAdd(&g_lane_stamps[q], (unsigned long long)st_acc[q]);
        atomicAdd(&g_lane_stamps[8], 1ull);
        for (int q = 0; q < 11; ++q) atomicAdd(&g_lane_stamps[9 + q], (unsigned long long)st_cnt[q]);
    }
#endif
}

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
