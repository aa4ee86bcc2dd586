// draw_wide.inc -- the batch LEGACY draw kernel for large pools (included by csa_legacy.hip after
// draw_lane.inc, inside its anonymous namespace; uses DrawArgs, select_bit, partner, dpp,
// raise_status, the outcome enum and draw_lane.inc's packed-key helpers and philox_lane).
//
// draw_lane_kernel's design carried to BASELINE config 5's shape (n = 8192, F = 40, k = 200):
// G = 8 lanes per panel (8 panels per wavefront), each lane holding in registers the packed
// (need, remaining) keys of FPL features and WPL = W / 8 words of the remaining pool; the pick
// lists go out in 16-byte chunks exactly as draw_lane_kernel writes them (same picks16 layout,
// same picks_pack_kernel).  What changes with the width:
//   * find_max_ratio_cat (legacy.py:124-157): the strict cross-multiplied argmax over the lane's
//     features, then a log2(G)-level DPP butterfly (lowest feature index on ties);
//   * holder scan (legacy.py:186-197): every lane counts the remaining holders of f* in its words,
//     an inclusive prefix across the group (DPP row_shr) tells the lane that holds the r-th one,
//     which finds the word and select_bit's it (its word masks and counts stay in registers);
//   * delete_person (legacy.py:103-120): the pick's features are read off the feature rows (one
//     LDS bit test per lane feature: no n-entry person-mask table, whose 64 KB would halve the
//     resident workgroups at n = 8192);
//   * delete_all_in_cat (legacy.py:47-62): cascading groups stage D = remaining & OR(rows of
//     their full features) in per-wave LDS slots; lane g of the wave then counts
//     popcount(D & featmask[g]) over the W words of two slots at a time (F <= 64).
// Same deferred post-pick SelectionError tests and lockstep Philox blocks as draw_lane_kernel
// (its header); F <= 64, W <= 16 G, no max = 0 < min feature (draw_kernel covers the rest).

constexpr int kWideThreads = 512;
constexpr int kWideSlots = 2;  // cascading groups per cooperative round (~0.25 cascades per wave-step at n = 8192)

__host__ __device__ inline size_t wide_lds_bytes(int G, int FPL, int WPL) {
    const size_t FN = (size_t)G * FPL, WN = (size_t)G * WPL, WNP = WN + WN / 16, LS = WNP + 1;
    return FN * LS * 8                                             // feature rows (padded, odd stride)
           + (size_t)4 * 64 * 4                                    // need0, rem0, mnx, pad (<= 64 features)
           + WN * 8                                                // attempt-start pool
           + (size_t)(kWideThreads / 64) * kWideSlots * WNP * 8    // cascade slots (padded)
           + (size_t)(kWideThreads / 64) * kWideSlots * 64 * 4;    // cascade decrements
}

// group-wide reductions over G = 8 / 16 lanes (DPP butterflies)
template <int G>
__device__ __forceinline__ int wmax(int v) {
    v = max(v, partner<0>(v));
    v = max(v, partner<1>(v));
    v = max(v, partner<2>(v));
    if constexpr (G >= 16) v = max(v, partner<3>(v));
    return v;
}
template <int G>
__device__ __forceinline__ uint32_t wor(uint32_t v) {
    v |= (uint32_t)partner<0>((int)v);
    v |= (uint32_t)partner<1>((int)v);
    v |= (uint32_t)partner<2>((int)v);
    if constexpr (G >= 16) v |= (uint32_t)partner<3>((int)v);
    return v;
}
// inclusive prefix sum inside the group: row_shr 1, 2, 4 (, 8), cross-group sources masked
template <int G>
__device__ __forceinline__ int wscan(int v, int glane) {
    v += dpp<0x111, 0xF, true>(0, v) & (glane >= 1 ? -1 : 0);
    v += dpp<0x112, 0xF, true>(0, v) & (glane >= 2 ? -1 : 0);
    v += dpp<0x114, 0xF, true>(0, v) & (glane >= 4 ? -1 : 0);
    if constexpr (G >= 16) v += dpp<0x118, 0xF, true>(0, v) & (glane >= 8 ? -1 : 0);
    return v;
}
// one butterfly level of the group argmax over packed keys (lowest feature index on ties)
template <int LVL>
__device__ __forceinline__ void wargmax_level(int &best, int &bi) {
    const int ob = partner<LVL>(best), oi = partner<LVL>(bi);
    const short2_t a = as_s2(ob), b = as_s2(best);
    const int l = (int)a.x * (int)b.y, r = (int)b.x * (int)a.y;
    const bool take = (l > r) | ((l == r) & (oi < bi));
    best = take ? ob : best;
    bi = take ? oi : bi;
}

template <int G, int FPL, int WPL>
__global__ __launch_bounds__(kWideThreads, 4) void draw_wide_kernel(DrawArgs A) {
    // Rows and cascade slots hold pool word w at w + w / 16 (one padding word after every 16): lane g
    // of a group reads words wbase..wbase + WPL - 1 of one row, so without the padding the 8 lanes of a
    // group start 16 words = 32 dwords apart and all hit one bank of the 32 a ds_read2_b64 uses
    // (an 8-way conflict; PMC: 7.4 conflict cycles per LDS instruction at n = 8192); with it they
    // start 34 dwords apart, on 8 different bank pairs.
    constexpr int FN = G * FPL, WN = G * WPL, WNP = WN + WN / 16, LS = WNP + 1;
    auto PH = [](int w) { return w + (w >> 4); };
    static_assert((G == 8 || G == 16) && FN <= 64 && FPL >= 1 && WPL >= 2 && (WPL % 2) == 0, "wide draw layout");
    extern __shared__ uint64_t smem[];
    const int F = A.F, W = A.W, k = A.k;
    uint64_t *fm = smem;
    const uint32_t *fm32 = reinterpret_cast<const uint32_t *>(fm);
    int32_t *need0_s = reinterpret_cast<int32_t *>(fm + FN * LS);
    int32_t *rem0_s = need0_s + 64, *mnx_s = need0_s + 128;
    uint64_t *pres0_s = reinterpret_cast<uint64_t *>(need0_s + 256);
    uint64_t *slot_all = pres0_s + WN;
    int32_t *dec_all = reinterpret_cast<int32_t *>(slot_all + (kWideThreads / 64) * kWideSlots * WNP);

    uint64_t live = 0;  // features with max > 0 (dead min = max = 0 features are removed)
    for (int f = 0; f < F; ++f) live |= (uint64_t)(A.fmax[f] != 0) << f;
    for (int t = threadIdx.x; t < FN * LS; t += blockDim.x) {
        const int f = t / LS, pw = t - f * LS, w = pw - pw / 17;  // pw % 17 == 16: a padding word
        if (pw % 17 == 16) {
            fm[t] = 0ull;
            continue;
        }
        fm[t] = (f < F && w < W && ((live >> f) & 1ull)) ? A.featmask[f * A.Ws + w] : 0ull;
    }
    for (int t = threadIdx.x; t < 64; t += blockDim.x) {
        const bool v = t < F && ((live >> t) & 1ull);
        need0_s[t] = v ? A.fmin[t] - A.sel0[t] : 0;
        rem0_s[t] = v ? A.rem0[t] : 0;
        mnx_s[t] = v ? A.fmin[t] - A.fmax[t] + 1 : -(1 << 30);  // need < mnx <=> selected == max
    }
    for (int t = threadIdx.x; t < WN; t += blockDim.x) pres0_s[t] = t < W ? A.present0[t] : 0ull;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int glane = lane & (G - 1), gbase = lane & ~(G - 1);
    const int fbase = glane * FPL, wbase = glane * WPL;
    uint64_t *slots = slot_all + (size_t)wave * kWideSlots * WNP;
    int32_t *decs = dec_all + wave * kWideSlots * 64;
    const uint32_t key0 = (uint32_t)A.seed, key1 = (uint32_t)(A.seed >> 32);
    const uint64_t n_groups = (uint64_t)__builtin_amdgcn_readfirstlane(gridDim.x * (blockDim.x / G));
    uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / G) + (threadIdx.x / G);
    bool active = i < A.n_panels;
    if (active && __hip_atomic_load(&A.status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) active = false;
    bool started = false;
    uint32_t a = 0;
    int s = 0;
    const int kpad = (k + 7) & ~7;
    int key[FPL];
    uint64_t rm[WPL];
    uint64_t pacc = 0ull;
#pragma unroll
    for (int j = 0; j < FPL; ++j) key[j] = 0;
#pragma unroll
    for (int j = 0; j < WPL; ++j) rm[j] = 0ull;
    uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;

    for (uint32_t it = 0; __ballot(active) != 0ull; ++it) {
        if ((it & 3u) == 0u) {  // attempt starts (analysis.py:147-148) + the Philox block of 4 steps
            if (active && !started) {
#pragma unroll
                for (int j = 0; j < FPL; ++j) key[j] = kpack(need0_s[fbase + j], rem0_s[fbase + j]);
#pragma unroll
                for (int j = 0; j < WPL; ++j) rm[j] = pres0_s[wbase + j];
                started = true;
                s = 0;
                pacc = 0ull;
            }
            const uint64_t panel = A.panel_begin + i;
            x0 = (uint32_t)s >> 2;
            x1 = A.attempt_base + a;
            x2 = (uint32_t)panel;
            x3 = (uint32_t)(panel >> 32);
            philox_lane(x0, x1, x2, x3, key0, key1);
        }

        int outcome = kContinue;
        uint64_t fl = 0;  // full features of the pick (bit g = feature g), group-wide
        if (started) {
            constexpr int kSentinel = (1 << 16) | 0xFF9C;  // need -100, remaining 1 (legacy.py:125)
            int best = kSentinel, bi = 0;  // lane-local index (inline constants in the selects)
#pragma unroll
            for (int j = 0; j < FPL; ++j) {
                const bool t = kbeats(key[j], best);
                best = t ? key[j] : best;
                bi = t ? j : bi;
            }
            bi += fbase;
            wargmax_level<0>(best, bi);
            wargmax_level<1>(best, bi);
            wargmax_level<2>(best, bi);
            if constexpr (G >= 16) wargmax_level<3>(best, bi);
            const int bn = kneed(best), bd = krem(best);
            if ((bd == 0) | (bn > bd)) {
                outcome = kFail;  // legacy.py:132-137
            } else if (best == kSentinel) {
                bool ne = false;
#pragma unroll
                for (int j = 0; j < WPL; ++j) ne |= rm[j] != 0ull;
                // KeyError (legacy.py:188), or the previous step's deferred emptied-pool error
                outcome = (wmax<G>((int)ne) || s == 0) ? kNoCandidate : kFail;
            } else {
                const int q = (int)(it & 3u);
                const uint32_t word = q == 0 ? x0 : (q == 1 ? x1 : (q == 2 ? x2 : x3));
                const int r = 1 + (int)__umulhi(word, (uint32_t)bd);  // randint(1, rem[f*]), legacy.py:149
                const uint64_t *row = fm + bi * LS + PH(wbase);  // WPL divides 16: the lane's words are contiguous
                uint64_t m[WPL];
                int cum[WPL], cnt = 0;  // cum[j]: holders of f* in this lane's words 0..j
#pragma unroll
                for (int j = 0; j < WPL; ++j) m[j] = row[j];  // every row read before the first use
#pragma unroll
                for (int j = 0; j < WPL; ++j) {
                    m[j] &= rm[j];
                    cnt = bcnt_acc((uint32_t)(m[j] >> 32), bcnt_acc((uint32_t)m[j], cnt));
                    cum[j] = cnt;
                }
                const int incl = wscan<G>(cnt, glane);
                const int rr = r - (incl - cnt);  // rank sought among this lane's words
                const bool hit = (rr >= 1) & (rr <= cnt);
                // the word PAIR whose preceding holder count is < rr (both masked words kept), then one
                // compare picks the word (as draw_lane_kernel: the selects once per two words).  (A
                // per-group LDS scratch the hit lane parks its words in, the pair read back by index,
                // removed the 48 selects but measured slower: draw 22.8 vs 20.7 ms per 10^6 panels at
                // n = 8192 -- the write / read round trip sits on the pick's critical path.)
                int base = 0, wsp = 0;
                uint64_t ma = m[0], mb = m[1];
#pragma unroll
                for (int j = 2; j < WPL; j += 2) {
                    const bool tk = cum[j - 1] < rr;
                    base = tk ? cum[j - 1] : base;
                    wsp = tk ? j : wsp;
                    ma = tk ? m[j] : ma;
                    mb = tk ? m[j + 1] : mb;
                }
                const int c0 = __popcll(ma);
                const bool second = rr - base > c0;
                const uint64_t ms = second ? mb : ma;
                const int ws = wsp + (int)second;
                const int b = select_bit(ms, hit ? rr - base - (second ? c0 : 0) : 1);
                const int p = wmax<G>(hit ? (wbase + ws) * 64 + b : -1);
                const int wi = p >> 6, bp = p & 31, hw = (p >> 5) & 1;
                uint32_t hb = 0;  // the pick's features among this lane's (bit j = feature fbase + j)
#pragma unroll
                for (int j = 0; j < FPL; ++j) hb |= ((fm32[2 * ((fbase + j) * LS + PH(wi)) + hw] >> bp) & 1u) << j;
                uint32_t em = 0;
#pragma unroll
                for (int j = FPL - 1; j >= 0; --j) {
                    const int hneg = -(int)((hb >> j) & 1u);
                    key[j] = as_i(as_s2(key[j]) + (short2_t)(short)hneg);
                    const uint32_t t = (uint32_t)(kneed(key[j]) - mnx_s[fbase + j]);  // broadcast LDS read
                    em = __builtin_amdgcn_alignbit(em, t, 31);
                }
                const uint32_t full = em & hb;
                // drop the pick from the register pool without a branch (owner lane: word ws): one bfe
                // + two v_bitop3 per word, as draw_lane_kernel
                {
                    const uint32_t M = hit ? 1u << ws : 0u;
                    const uint32_t bit = 1u << ((uint32_t)b & 31u), Blo = b < 32 ? bit : 0u, Bhi = b < 32 ? 0u : bit;
#pragma unroll
                    for (int j = 0; j < WPL; ++j) {
                        const uint32_t sel = (uint32_t)((int)(M << (31 - j)) >> 31);
                        const uint32_t lo = (uint32_t)rm[j] & ~(Blo & sel);
                        const uint32_t hi = (uint32_t)(rm[j] >> 32) & ~(Bhi & sel);
                        rm[j] = ((uint64_t)hi << 32) | lo;
                    }
                }
                {  // pick list: 8 picks per 16-byte chunk (lanes 0 and 1 of the group), as draw_lane_kernel
                    const int slot = s & 7;
                    if ((slot >> 2) == glane) pacc |= (uint64_t)(uint16_t)p << (16 * (slot & 3));
                    if (((slot == 7) | (s == k - 1)) & (glane < 2)) {
                        *reinterpret_cast<uint64_t *>(A.picks16 + i * (uint64_t)kpad + (s & ~7) + 4 * glane) = pacc;
                        pacc = 0ull;
                    }
                }
                const uint64_t mine = (uint64_t)full << fbase;
                fl = ((uint64_t)wor<G>((uint32_t)(mine >> 32)) << 32) | wor<G>((uint32_t)mine);
            }
        }

        // ---- the k-th pick: check_min_cats (legacy.py:160-168, analysis.py:155-159) now, and no
        // cascade for a panel that passes (see draw_lane_kernel): an under-quota panel still cascades
        // when the statistics are wanted
        const bool last = started & (outcome == kContinue) & (s == k - 1);
        if (__ballot(last) != 0ull) {
            bool u = false;
#pragma unroll
            for (int j = 0; j < FPL; ++j) u |= kneed(key[j]) > 0;
            const bool under = wmax<G>((int)u) != 0;
            if (last) {
                outcome = under ? kReject : kAccept;
                if (!(under && A.stats)) fl = 0ull;
            }
        }

        // ---- delete_all_in_cat, wave-cooperative in rounds of kWideSlots cascading groups --------
        uint64_t cb = __ballot((fl != 0ull) && glane == 0);
        while (cb) {
            uint64_t rb = cb;  // usually all of them fit one round
            if (__popcll(cb) > kWideSlots) {
                rb = 0ull;
#pragma unroll
                for (int j = 0; j < kWideSlots; ++j) {
                    const uint64_t low = cb & (~cb + 1ull);
                    rb |= low;
                    cb ^= low;
                }
            } else {
                cb = 0ull;
            }
            const bool owner = (rb >> gbase) & 1ull;
            // set bits of rb below the group's first lane (rb holds first lanes only)
            const int slot = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(rb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rb, 0u)) -
                             (glane ? (int)owner : 0);
            if (owner) {
                // remaining &= ~OR(rows of the full features), this lane's words; the slot receives the
                // new pool and the counting pass recounts every feature's remaining (as draw_lane_kernel)
                uint64_t bits = fl;
                uint64_t orr[WPL];
                const uint64_t *f0 = fm + (__ffsll((unsigned long long)bits) - 1) * LS + PH(wbase);
                bits &= bits - 1ull;
#pragma unroll
                for (int j = 0; j < WPL; ++j) orr[j] = f0[j];
                while (bits) {
                    const uint64_t *fr = fm + (__ffsll((unsigned long long)bits) - 1) * LS + PH(wbase);
                    bits &= bits - 1ull;
#pragma unroll
                    for (int j = 0; j < WPL; ++j) orr[j] |= fr[j];
                }
                uint64_t *srow = slots + slot * WNP + PH(wbase);
#pragma unroll
                for (int j = 0; j < WPL; ++j) {
                    rm[j] &= ~orr[j];
                    srow[j] = rm[j];
                }
            }
            // rem[g] = popcount(pool & featmask[g]), the words of each feature split over lanes so that
            // every lane counts about FN * WN / 64 words (one lane per feature over all WN words left 24
            // of 64 lanes idle at F = 40 and counted 128 words each): pass A, features 0..31, two word
            // halves (lane = feature + 32 half); pass B (FN > 32), features 32..FN-1, NBP = pow2 >= FN - 32
            // of them, 64 / NBP word parts (lane = feature - 32 + NBP part); partial sums meet by
            // permlane swaps / DPP
            const int ns = __popcll(rb);
            constexpr int NB = FN > 32 ? FN - 32 : 0;
            constexpr int NBP = NB <= 8 ? 8 : NB <= 16 ? 16 : 32;
            constexpr int PB = 64 / NBP, WA = WN / 2, WB = WN / PB;  // words per lane in each pass
            static_assert(WA % 4 == 0 && WB % 4 == 0, "count pass word ranges");
            const int ga = lane & 31, gb = 32 + (lane & (NBP - 1));
            const uint64_t *frow_a = fm + (ga < FN ? ga : 0) * LS;
            const uint64_t *frow_b = fm + (gb < FN ? gb : 0) * LS;
            const int wa0 = (lane >> 5) * WA, wb0 = (lane / NBP) * WB;
            // counts of one word range of one row against one or two slots
            auto count_range = [&](const uint64_t *frow, const uint64_t *d0, const uint64_t *d1, int w_begin,
                                   auto nw_c, auto two_c, int &c0, int &c1) {
                constexpr int NW = decltype(nw_c)::value;
                constexpr bool TWO = decltype(two_c)::value;
                constexpr int CK = 4;  // words per batch of reads (CK divides 16: PH(w + u) = PH(w) + u)
#pragma unroll 4
                for (int t = 0; t < NW; t += CK) {
                    const int pw = PH(w_begin + t);
                    uint64_t fa[CK], a0[CK], a1[CK];
#pragma unroll
                    for (int u = 0; u < CK; ++u) {
                        fa[u] = frow[pw + u];
                        a0[u] = d0[pw + u];
                        if constexpr (TWO) a1[u] = d1[pw + u];
                    }
#pragma unroll
                    for (int u = 0; u < CK; ++u) {
                        const uint64_t x0 = a0[u] & fa[u];
                        c0 = bcnt_acc((uint32_t)(x0 >> 32), bcnt_acc((uint32_t)x0, c0));
                        if constexpr (TWO) {
                            const uint64_t x1 = a1[u] & fa[u];
                            c1 = bcnt_acc((uint32_t)(x1 >> 32), bcnt_acc((uint32_t)x1, c1));
                        }
                    }
                }
            };
            auto sum32 = [](int v) {  // + lane +- 32
                const auto s2 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
                return (int)(s2[0] + s2[1]);
            };
            auto sum_parts_b = [&](int v) {  // sum over the PB lanes of one pass-B feature
                if constexpr (NBP == 8) v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);  // row_ror:8
                if constexpr (NBP <= 16) {
                    const auto s2 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
                    v = (int)(s2[0] + s2[1]);
                }
                return sum32(v);
            };
            auto count_pass = [&](int q0, auto two_c) {
                constexpr bool TWO = decltype(two_c)::value;
                const uint64_t *d0 = slots + q0 * WNP, *d1 = d0 + WNP;
                int a0c = 0, a1c = 0;
                count_range(frow_a, d0, d1, wa0, std::integral_constant<int, WA>{}, two_c, a0c, a1c);
                a0c = sum32(a0c);
                if constexpr (TWO) a1c = sum32(a1c);
                if (lane < 32 && ga < FN) {  // remaining is the key's high half
                    decs[q0 * 64 + ga] = a0c << 16;
                    if constexpr (TWO) decs[(q0 + 1) * 64 + ga] = a1c << 16;
                }
                if constexpr (NB > 0) {
                    int b0c = 0, b1c = 0;
                    count_range(frow_b, d0, d1, wb0, std::integral_constant<int, WB>{}, two_c, b0c, b1c);
                    b0c = sum_parts_b(b0c);
                    if constexpr (TWO) b1c = sum_parts_b(b1c);
                    if (lane < NBP && gb < FN) {
                        decs[q0 * 64 + gb] = b0c << 16;
                        if constexpr (TWO) decs[(q0 + 1) * 64 + gb] = b1c << 16;
                    }
                }
            };
            int q0 = 0;
            for (; q0 + 1 < ns; q0 += 2) count_pass(q0, std::true_type{});
            if (q0 < ns) count_pass(q0, std::false_type{});
            if (owner) {
                const int32_t *dv = decs + slot * 64 + fbase;
#pragma unroll
                for (int j = 0; j < FPL; ++j) key[j] = (key[j] & 0xFFFF) | dv[j];  // remaining recounted
            }
        }

        // ---- bookkeeping: the k-th pick's min-quota check, restarts, accepted panels -------------
        if (started) {
            if (outcome == kContinue) ++s;  // (the k-th pick's outcome was set before the cascades)
            if (outcome != kContinue) {
                const uint64_t panel = A.panel_begin + i;
                started = false;
                s = 0;
                if (outcome == kNoCandidate) {
                    if (glane == 0) raise_status(A.status, CSA_E_NO_CANDIDATE, panel);
                    active = false;
                } else if (outcome != kAccept) {  // SelectionError restart / min-quota rejection
                    if (A.stats) {
                        // a feature with remaining == 0 and selected < min after the k-th pick is the
                        // reference's SelectionError (legacy.py:55, 73; the test is deferred here)
                        int rj = outcome == kReject;
                        if (rj) {
                            bool dead = false;
#pragma unroll
                            for (int j = 0; j < FPL; ++j) dead |= kneed(key[j]) > 0 && krem(key[j]) == 0;
                            rj = !wmax<G>((int)dead);
                        }
                        if (glane == 0) atomicAdd(A.stats + rj, 1ull);
                    }
                    if (++a >= A.max_attempts) {
                        if (glane == 0) raise_status(A.status, CSA_E_ATTEMPT_LIMIT, panel);
                        active = false;
                    }
                } else {
                    if (A.attempts && glane == 0) A.attempts[i] = a + 1;
                    i += n_groups;
                    a = 0;
                    active = i < A.n_panels;
                }
            }
        }
    }
}
