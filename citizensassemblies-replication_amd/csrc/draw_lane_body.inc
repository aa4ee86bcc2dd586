// draw_lane_body.inc -- the function body of draw_lane_kernel and of its household form
// draw_lane_hh_kernel, included once under each entry point's signature by draw_lane.inc with
// CSA_DRAW_HH = 0 / 1 (one text, two kernels: see draw_solo_body.inc).
{
#if CSA_DRAW_HH
    constexpr int NP = 8;  // the household forms keep all 8 slack planes
#endif
    constexpr bool HH = CSA_DRAW_HH;
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
    [[maybe_unused]] uint16_t *ring = reinterpret_cast<uint16_t *>(dec_all + (kLaneThreads / 64) * kLaneSlots * FN);
    if constexpr (HH) {
        for (int t = threadIdx.x; t < n; t += kLaneThreads) ring[t] = (uint16_t)A.addr_next[t];
        __syncthreads();
    }

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
        [[maybe_unused]] int hp = -1;  // HH: this step's pick (both lanes), whose household leaves the pool below
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
                if constexpr (HH) hp = p;
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
                if (!(under && A.stats)) {
                    fl = 0u;
                    if constexpr (HH) hp = -1;  // the household's deletion runs under the cascades' condition
                }
            }
        }

        // ---- HH: the pick's household leaves the pool unpicked (legacy.py:109-113).  Both lanes of a
        // pair hold the same pick and walk its ring in step (at most n agents: a list that is no ring
        // cannot hold the wave); position m of agent q in this lane's order is q (first lane) or
        // 64 WN - 1 - q (second lane, mirrored), and the lane owns it when m < 64 WPL --------------
        if constexpr (HH) {
            if (hp >= 0) {
                int q = ring[hp];
                for (int guard = 0; q != hp && guard < n; q = ring[q], ++guard) {
                    const int m = poff + psgn * q;
                    const int wq = m >> 6;  // >= WPL on the lane that does not hold q: matches no word
                    const uint64_t qb = 1ull << (m & 63);
                    bool there = false;
#pragma unroll
                    for (int j = 0; j < WPL; ++j) {
                        if (wq == j) {
                            there = (rm[j] & qb) != 0ull;
                            rm[j] &= ~qb;
                        }
                    }
                    if (max((int)there, partner<0>((int)there))) {  // remaining drops for each of the mate's features
                        const uint32_t hq = pm[q] >> fbase;
#pragma unroll
                        for (int j = 0; j < FPL; ++j) key[j] -= (int)(((hq >> j) & 1u) << 16);
                    }
                }
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
