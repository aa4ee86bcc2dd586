// draw_solo_body.inc -- the function body of draw_solo_kernel and of its household form
// draw_solo_hh_kernel, included once under each entry point's signature by draw_solo.inc with
// CSA_DRAW_HH = 0 / 1.  One text, two kernels: the household steps stand under `if constexpr (HH)`,
// and the existing entry point compiles to the code it had when it held this body itself (as a shared
// __device__ function the body's reads of blockDim / gridDim, and those of the pack it calls, compile
// differently, and every existing kernel's code changed: DESIGN 4.17).
{
#if CSA_DRAW_HH
    constexpr int NP = 8;  // the household forms keep all 8 slack planes
#endif
    constexpr bool HH = CSA_DRAW_HH;
    constexpr int LS = WN + 1;        // odd row stride
    constexpr bool kSlackPlanes = FN >= 16;
    static_assert(FN <= 32 && WN <= 32 && (FN % 8) == 0 && (WN % 2) == 0 && NP >= 1 && NP <= 8, "solo draw layout");
    extern __shared__ uint64_t smem[];
    const int n = A.n, k = A.k;
    const DrawImage L = draw_image_layout(false, FN, WN, n);
    uint64_t *fm = smem;
    uint32_t *pm = reinterpret_cast<uint32_t *>(fm + L.pm);
    int32_t *need0_s = reinterpret_cast<int32_t *>(fm + L.need0);
    int32_t *rem0_s = need0_s + FN, *mnx_s = need0_s + 2 * FN;
    uint64_t *pres0_s = fm + L.pres0;
    uint64_t *slot_all = fm + L.words;
    int32_t *cnt_all = reinterpret_cast<int32_t *>(slot_all + (kSoloThreads / 64) * kSoloSlots * WN);

    // everything below slot_all is the instance's image (draw_image_build, as draw_lane_kernel): dead
    // features removed, the start keys packed, and mnx_s the slack of every feature, bit-sliced (FN >= 16:
    // mnx_s[i] bit j = bit i of the slack of feature j, dead and padding features all ones), or
    // mnx_s[f] = min - max + 1 (FN = 8)
    load_draw_image(smem, A.image, L.words / 2);
    [[maybe_unused]] uint16_t *ring = reinterpret_cast<uint16_t *>(cnt_all + (kSoloThreads / 64) * kSoloSlots * FN);
    if constexpr (HH) {
        for (int t = threadIdx.x; t < n; t += kSoloThreads) ring[t] = (uint16_t)A.addr_next[t];
        __syncthreads();
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *slots = slot_all + (size_t)wave * kSoloSlots * WN;
    int32_t *cnts = cnt_all + wave * kSoloSlots * FN;
    const uint32_t key0 = (uint32_t)A.seed, key1 = (uint32_t)(A.seed >> 32);
    const uint64_t n_lanes = (uint64_t)__builtin_amdgcn_readfirstlane(gridDim.x * blockDim.x);
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool active = i < A.n_panels;
    if (active && __hip_atomic_load(&A.status[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) active = false;
    bool started = false;
    uint32_t a = 0;
    int s = 0;
    int key[FN];       // packed (need, remaining) per feature
    uint64_t rm[WN];   // remaining pool
    uint64_t pacc = 0ull;  // picks of steps 4c .. 4c + 3 (u16 each), stored per 4 steps
    uint32_t sp[NP];       // slack bit planes (FN >= 16)
#pragma unroll
    for (int q = 0; q < NP; ++q) sp[q] = 0u;
    const int kpad = (k + 7) & ~7;
#pragma unroll
    for (int j = 0; j < FN; ++j) key[j] = 0;
#pragma unroll
    for (int j = 0; j < WN; ++j) rm[j] = 0ull;
    uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;

    for (uint32_t it = 0; __ballot(active) != 0ull; ++it) {
        // ---- attempt starts (analysis.py:147-148) + the Philox block of the next 4 steps ----------
        if ((it & 3u) == 0u) {
            if (active && !started) {
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    key[j] = K8 ? need0_s[j] : kpack(need0_s[j], rem0_s[j]);  // K8: packed at kernel start
                if constexpr (kSlackPlanes) {
#pragma unroll
                    for (int q = 0; q < NP; ++q) sp[q] = (uint32_t)mnx_s[q];
                }
#pragma unroll
                for (int j = 0; j < WN; ++j) rm[j] = pres0_s[j];
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

        // ---- one step: find_max_ratio_cat + holder pick + delete_person -------------------------
        int outcome = kContinue;
        uint32_t fl = 0;  // the pick's features that reached max
        [[maybe_unused]] int hp = -1;  // HH: this step's pick, whose household leaves the pool below
        if (started) {
            constexpr int kSentinel = kDrawSentinel<K8>;  // need -100, remaining 1 (legacy.py:125)
            // four independent chains over consecutive feature ranges, merged in index order (ties
            // keep the lower chain: the first maximum, as the single strict-'>' chain)
            constexpr int Q = FN / 4;
            int best, bi;
            if constexpr (K8) {
                // 8-bit need keys carrying their index (draw_lane.inc, K8): one select per feature
                int b0 = kSentinel, b1 = kSentinel, b2 = kSentinel, b3 = kSentinel;
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    const bool t0 = k8beats(key[j], b0), t1 = k8beats(key[Q + j], b1);
                    const bool t2 = k8beats(key[2 * Q + j], b2), t3 = k8beats(key[3 * Q + j], b3);
                    b0 = t0 ? key[j] : b0;
                    b1 = t1 ? key[Q + j] : b1;
                    b2 = t2 ? key[2 * Q + j] : b2;
                    b3 = t3 ? key[3 * Q + j] : b3;
                }
                const int ba = k8beats(b1, b0) ? b1 : b0, bb = k8beats(b3, b2) ? b3 : b2;
                best = k8beats(bb, ba) ? bb : ba;
                bi = k8idx1(best);  // index + 1: the row base below is one row early
            } else {
                int b0 = kSentinel, i0 = 0, b1 = kSentinel, i1 = Q, b2 = kSentinel, i2 = 2 * Q, b3 = kSentinel, i3 = 3 * Q;
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    const bool t0 = kbeats(key[j], b0), t1 = kbeats(key[Q + j], b1);
                    const bool t2 = kbeats(key[2 * Q + j], b2), t3 = kbeats(key[3 * Q + j], b3);
                    b0 = t0 ? key[j] : b0;
                    i0 = t0 ? j : i0;
                    b1 = t1 ? key[Q + j] : b1;
                    i1 = t1 ? Q + j : i1;
                    b2 = t2 ? key[2 * Q + j] : b2;
                    i2 = t2 ? 2 * Q + j : i2;
                    b3 = t3 ? key[3 * Q + j] : b3;
                    i3 = t3 ? 3 * Q + j : i3;
                }
                const bool ta = kbeats(b1, b0), tb = kbeats(b3, b2);
                const int ba = ta ? b1 : b0, ia = ta ? i1 : i0, bb = tb ? b3 : b2, ib = tb ? i3 : i2;
                const bool tc = kbeats(bb, ba);
                best = tc ? bb : ba;
                bi = tc ? ib : ia;
            }
            const int bn = K8 ? k8need(best) : kneed(best), bd = krem(best);
            if ((bd == 0) | (bn > bd)) {
                outcome = kFail;  // legacy.py:132-137
            } else if (best == kSentinel) {
                bool ne = false;
#pragma unroll
                for (int j = 0; j < WN; ++j) ne |= rm[j] != 0ull;
                // KeyError (legacy.py:188), or the previous step's deferred emptied-pool error
                outcome = (ne || s == 0) ? kNoCandidate : kFail;
            } else {
                const int q = (int)(it & 3u);  // == s & 3 for every running lane
                const uint32_t word = q == 0 ? x0 : (q == 1 ? x1 : (q == 2 ? x2 : x3));
                const int r = 1 + (int)__umulhi(word, (uint32_t)bd);  // randint(1, rem[f*]), legacy.py:149
                const uint64_t *row = (K8 ? fm - LS : fm) + bi * LS;
                // forward scan over word pairs: the pair whose preceding holder count is < r is kept
                // (both masked words and the count before it); row reads in batches of RB words.
                // `acc < r` is monotone, so the keep runs under a narrowing lane predicate instead of
                // selects (draw_lane.inc): a lane leaves the scan at the first pair it does not take --
                // its r-th holder is in the pair it kept -- and under the predicate the masked words are
                // formed in place (the empty asm keeps the body from being turned back into selects).
                // Both guards -- this asm and the drop's scheduling barrier -- stop the compiler's
                // if-conversion and nothing else; after a compiler update, tools/kernel_regs.sh and the
                // v_cndmask / v_bitop3 count of the step loop's ISA say whether they still do (a failure
                // is slower, not wrong).
                // kPredicated: <16, 28, 5, true> is the one FN = 16 form that fits 4 waves per SIMD
                // (128 VGPRs; the launch bounds ask for 3) and either predicated block costs it that
                // wave (139 / 129 VGPRs), so it keeps the selects and the v_bitop3 drop -- and select_bit's
                // search down to single bits, whose nibble table costs it the same wave.
                constexpr bool kPredicated = !(FN == 16 && WN == 28 && NP == 5 && K8);
                int acc = 0, base = 0, wsp = 0;
                uint64_t ma = 0ull, mb = 0ull;
                constexpr int RB = 4;  // 4-word row batches: FN = 8 fits 128 VGPRs without spills (8: a few, -0.9 %)
#pragma unroll
                for (int j0 = 0; j0 < WN; j0 += RB) {
                    uint64_t rw[RB];
#pragma unroll
                    for (int u = 0; u < RB; ++u) rw[u] = j0 + u < WN ? row[j0 + u] : 0ull;
#pragma unroll
                    for (int u = 0; u < RB && j0 + u < WN; u += 2) {
                        const int j = j0 + u;
                        if constexpr (kPredicated) {
                            if (j > 0 && !(acc < r)) goto scanned;  // (r >= 1: the first pair is always taken)
                            base = acc;
                            wsp = j;
                            ma = rm[j] & rw[u];
                            mb = rm[j + 1] & rw[u + 1];
                            asm("" : "+v"(ma), "+v"(mb));
                            acc = bcnt_acc((uint32_t)(ma >> 32), bcnt_acc((uint32_t)ma, acc));
                            acc = bcnt_acc((uint32_t)(mb >> 32), bcnt_acc((uint32_t)mb, acc));
                        } else {
                            const uint64_t m0 = rm[j] & rw[u], m1 = rm[j + 1] & rw[u + 1];
                            const bool tk = acc < r;
                            base = tk ? acc : base;
                            wsp = tk ? j : wsp;
                            ma = tk ? m0 : ma;
                            mb = tk ? m1 : mb;
                            acc = bcnt_acc((uint32_t)(m0 >> 32), bcnt_acc((uint32_t)m0, acc));
                            acc = bcnt_acc((uint32_t)(m1 >> 32), bcnt_acc((uint32_t)m1, acc));
                        }
                    }
                }
            [[maybe_unused]] scanned:
                const int c0 = __popcll(ma);
                const bool second = r - base > c0;  // the holder is in the pair's second word
                const uint64_t ms = second ? mb : ma;
                const int ws = wsp + (int)second;
                const int b = select_bit<kPredicated>(ms, r - base - (second ? c0 : 0));  // (129 VGPRs with the nibble table)
                const int p = ws * 64 + b;
                if constexpr (HH) hp = p;
                const uint32_t hb = pm[p];
                // drop the pick from the register pool while the pm[p] read is in flight (none of it
                // needs the pick's features): the picked bit is set in rm[ws], so clearing it is adding
                // -(1 << b) = ~0 << b; the addends of a pair's two words are formed once (the other
                // word's is 0) and each pair adds them under its own lane predicate -- a compare and
                // two v_lshl_add_u64 per pair instead of a bfe + two v_bitop3 per word (draw_lane.inc)
                if constexpr (kPredicated) {
                    const uint64_t nb = ~0ull << b;
                    const uint64_t dA = second ? 0ull : nb, dB = second ? nb : 0ull;
#pragma unroll
                    for (int j = 0; j < WN; j += 2) {
                        if (wsp == j) {
                            rm[j] += dA;
                            rm[j + 1] += dB;
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                } else {  // branch-free: one bfe (the word's select mask) + one v_bitop3 per dword
                    const uint32_t M = 1u << ws;
                    const uint32_t bit = 1u << ((uint32_t)b & 31u), Blo = b < 32 ? bit : 0u, Bhi = b < 32 ? 0u : bit;
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        const uint32_t sel = (uint32_t)((int)(M << (31 - j)) >> 31);
                        const uint32_t lo = (uint32_t)rm[j] & ~(Blo & sel);
                        const uint32_t hi = (uint32_t)(rm[j] >> 32) & ~(Bhi & sel);
                        rm[j] = ((uint64_t)hi << 32) | lo;
                    }
                }
                pacc |= (uint64_t)(uint16_t)p << (16 * q);
                if constexpr (kSlackPlanes) {
#pragma unroll
                    for (int j = 0; j < FN; ++j) {
                        const int hneg = (int)(hb << (31 - j)) >> 31;  // -has
                        key[j] = as_i(as_s2(key[j]) + (short2_t)(short)hneg);
                    }
                    // selected == max after this pick (legacy.py:113-114) <=> slack max - selected
                    // reaches 0: bit-sliced decrement of the pick's features, then a zero test
                    constexpr uint32_t kFnMask = FN >= 32 ? 0xFFFFFFFFu : (1u << FN) - 1u;
                    uint32_t bw = hb & kFnMask;
                    const uint32_t picked = bw;
                    uint32_t nz = 0u;
#pragma unroll
                    for (int qq = 0; qq < NP; ++qq) {
                        const uint32_t t = sp[qq];
                        sp[qq] = t ^ bw;
                        nz |= sp[qq];
                        if (qq + 1 < NP) bw &= ~t;
                    }
                    fl = picked & ~nz;
                } else {
                    uint32_t em = 0;
#pragma unroll
                    for (int j = FN - 4; j >= 0; j -= 4) {
                        const int4 mv = *reinterpret_cast<const int4 *>(mnx_s + j);  // broadcast LDS read
                        const int mx[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
                        for (int u = 3; u >= 0; --u) {
                            const int hneg = (int)(hb << (31 - (j + u))) >> 31;
                            key[j + u] = as_i(as_s2(key[j + u]) + (short2_t)(short)hneg);
                            const uint32_t t = (uint32_t)((K8 ? k8need(key[j + u]) : kneed(key[j + u])) - mx[u]);
                            em = __builtin_amdgcn_alignbit(em, t, 31);
                        }
                    }
                    fl = em & hb;
                }
                // the pick joined its 4-step chunk above (s & 3 = it & 3 is wave-uniform: a scalar
                // shift amount); the chunk leaves as 8 bytes after its 4th step or the k-th
                if ((q == 3) | (s == k - 1)) {
                    // (chunked layout of the fused pack, draw_lane.inc: 256 panels x 4 picks per chunk)
                    const uint64_t off = A.panels ? ((uint64_t)blockIdx.x * (kpad >> 2) + (uint64_t)(s >> 2)) * 1024 +
                                                        4 * threadIdx.x
                                                  : i * (uint64_t)kpad + (s & ~3);
                    *reinterpret_cast<uint64_t *>(A.picks16 + off) = pacc;
                    pacc = 0ull;
                }
            }
        }

        // ---- the k-th pick: check_min_cats (legacy.py:160-168, analysis.py:155-159) now, and no
        // cascade for a panel that passes (see draw_lane_kernel): an under-quota panel still cascades
        // when the statistics are wanted
        const bool last = started & (outcome == kContinue) & (s == k - 1);
        if (__ballot(last) != 0ull) {
            bool under = false;
#pragma unroll
            for (int j = 0; j < FN; ++j) under |= (K8 ? k8need(key[j]) : kneed(key[j])) > 0;
            if (last) {
                outcome = under ? kReject : kAccept;
                if (!(under && A.stats)) {
                    fl = 0u;
                    if constexpr (HH) hp = -1;  // the household's deletion runs under the cascades' condition
                }
            }
        }

        // ---- HH: the pick's household leaves the pool unpicked (legacy.py:109-113), each lane walking
        // its own pick's ring until it is back at the pick (at most n agents: a list that is no ring
        // cannot hold the wave) ----------------------------------------------------------------------
        if constexpr (HH) {
            if (hp >= 0) {
                int q = ring[hp];
                for (int guard = 0; q != hp && guard < n; q = ring[q], ++guard) {
                    const int wq = q >> 6;
                    const uint64_t qb = 1ull << (q & 63);
                    bool there = false;
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        if (wq == j) {
                            there = (rm[j] & qb) != 0ull;
                            rm[j] &= ~qb;
                        }
                    }
                    if (there) {  // remaining (the key's high half) drops for each of the mate's features
                        const uint32_t hq = pm[q];
#pragma unroll
                        for (int j = 0; j < FN; ++j) key[j] -= (int)(((hq >> j) & 1u) << 16);
                    }
                }
            }
        }

        // ---- delete_all_in_cat, wave-cooperative in rounds of kSoloSlots cascading lanes ---------
        uint64_t cb = __ballot(fl != 0u);
        while (cb) {
            uint64_t rb = cb;
            if (__popcll(cb) > kSoloSlots) {
                rb = 0ull;
#pragma unroll
                for (int j = 0; j < kSoloSlots; ++j) {
                    const uint64_t low = cb & (~cb + 1ull);
                    rb |= low;
                    cb ^= low;
                }
            } else {
                cb = 0ull;
            }
            const bool mine = (rb >> lane) & 1ull;
            const int slot = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(rb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rb, 0u));
            if (mine) {
                // remaining &= ~OR(rows of the full features); the slot receives the NEW pool, whose
                // recount below is every feature's remaining outright (D is never formed)
                // (one full feature's row at a time, no OR temporary: a whole-row OR would hold
                // 2 WN more VGPRs; usually exactly one feature is full)
                uint64_t *srow = slots + slot * WN;
                uint32_t bits = fl;
                do {
                    const uint64_t *fr = fm + __builtin_ctz(bits) * LS;
                    bits &= bits - 1u;
#pragma unroll
                    for (int j = 0; j < WN; ++j) rm[j] &= ~fr[j];
                } while (bits);
#pragma unroll
                for (int j = 0; j < WN; ++j) srow[j] = rm[j];
            }
            // rem[g] = popcount(pool & featmask[g]): lane = (feature g, word part), P parts of WPP words
            // (P = 64 / FN where it divides WN: 8 parts of 4 words at FN = 8, W = 32, instead of 2 halves
            // of 16 words with 48 of the 64 lanes idle); the parts' counts meet by DPP row_ror:8 /
            // v_permlane16_swap / v_permlane32_swap (stride FN << level)
            constexpr int P0 = 64 / FN;
            constexpr int P = WN % P0 == 0 ? P0 : WN % (P0 / 2) == 0 ? P0 / 2 : WN % (P0 / 4) == 0 ? P0 / 4 : 1;
            constexpr int WPP = WN / P;
            static_assert(P >= 1 && WN % P == 0 && FN * P <= 64, "solo count-pass layout");
            const int g = lane & (FN - 1), part = lane / FN;
            const bool counting = part < P;
            const int w0 = (counting ? part : 0) * WPP;
            const uint64_t *frow = fm + g * LS;
            const int ns = __popcll(rb);
            auto sum_parts = [&](int v) {
                v = counting ? v : 0;
                if constexpr (FN == 8 && P > 1) v += __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);  // row_ror:8
                if constexpr (FN * P > 16) {
                    const auto s2 = __builtin_amdgcn_permlane16_swap(v, v, false, false);
                    v = (int)(s2[0] + s2[1]);
                }
                if constexpr (FN * P > 32) {
                    const auto s2 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
                    v = (int)(s2[0] + s2[1]);
                }
                return v;
            };
            auto count_pass = [&](int q0, auto two_c) {
                constexpr bool TWO = decltype(two_c)::value;
                const uint64_t *d0 = slots + q0 * WN, *d1 = d0 + WN;
                int c0 = 0, c1 = 0;
                constexpr int CK = 2;
#pragma unroll
                for (int t0 = 0; t0 < WPP; t0 += CK) {
                    uint64_t a0[CK], a1[CK], f[CK];
#pragma unroll
                    for (int u = 0; u < CK; ++u) {
                        const bool ok = t0 + u < WPP;
                        f[u] = ok ? frow[w0 + t0 + u] : 0ull;
                        a0[u] = ok ? d0[w0 + t0 + u] : 0ull;
                        a1[u] = (TWO && ok) ? d1[w0 + t0 + u] : 0ull;
                    }
#pragma unroll
                    for (int u = 0; u < CK; ++u) {
                        if (t0 + u < WPP) {
                            const uint64_t y0 = a0[u] & f[u];
                            c0 = bcnt_acc((uint32_t)(y0 >> 32), bcnt_acc((uint32_t)y0, c0));
                            if constexpr (TWO) {
                                const uint64_t y1 = a1[u] & f[u];
                                c1 = bcnt_acc((uint32_t)(y1 >> 32), bcnt_acc((uint32_t)y1, c1));
                            }
                        }
                    }
                }
                c0 = sum_parts(c0);
                if constexpr (TWO) c1 = sum_parts(c1);
                if (lane < FN) {  // remaining is the key's high half
                    cnts[q0 * FN + lane] = c0 << 16;
                    if constexpr (TWO) cnts[(q0 + 1) * FN + lane] = c1 << 16;
                }
            };
            int q0 = 0;
            for (; q0 + 1 < ns; q0 += 2) count_pass(q0, std::true_type{});
            if (q0 < ns) count_pass(q0, std::false_type{});
            if (mine) {
                const int32_t *dv = cnts + slot * FN;
#pragma unroll
                for (int j = 0; j < FN; j += 4) {
                    const int4 v = *reinterpret_cast<const int4 *>(dv + j);
                    key[j] = (key[j] & 0xFFFF) | v.x;
                    key[j + 1] = (key[j + 1] & 0xFFFF) | v.y;
                    key[j + 2] = (key[j + 2] & 0xFFFF) | v.z;
                    key[j + 3] = (key[j + 3] & 0xFFFF) | v.w;
                }
            }
        }

        // ---- bookkeeping: the k-th pick's min-quota check, restarts, accepted panels -------------
        if (started) {
            if (outcome == kContinue) ++s;  // (the k-th pick's outcome was set before the cascades)
            if (outcome != kContinue) {
                const uint64_t panel = A.panel_begin + i;
                started = false;  // the next attempt / panel starts at the next iteration it = 0 mod 4
                s = 0;
                if (outcome == kNoCandidate) {
                    raise_status(A.status, CSA_E_NO_CANDIDATE, panel);
                    active = false;
                } else if (outcome != kAccept) {  // SelectionError restart / min-quota rejection
                    if (A.stats) {
                        // a feature with remaining == 0 and selected < min after the k-th pick is the
                        // reference's SelectionError (legacy.py:55, 73; the test is deferred here)
                        bool dead = false;
                        if (outcome == kReject) {
#pragma unroll
                            for (int j = 0; j < FN; ++j)
                                dead |= (K8 ? k8need(key[j]) : kneed(key[j])) > 0 && krem(key[j]) == 0;
                        }
                        atomicAdd(A.stats + (outcome == kReject && !dead), 1ull);
                    }
                    if (++a >= A.max_attempts) {
                        raise_status(A.status, CSA_E_ATTEMPT_LIMIT, panel);
                        active = false;
                    }
                } else {  // picks16 holds this attempt's k picks (its last chunk was stored at s = k-1)
                    if (A.attempts) A.attempts[i] = a + 1;
                    i += n_lanes;
                    a = 0;
                    active = i < A.n_panels;
                }
            }
        }
    }

    // ---- fused pack: the workgroup's 256 panels in two 128-row tiles ----------------------------
    if (A.panels) {
        const uint64_t pb = (uint64_t)blockIdx.x * kSoloThreads;
#pragma unroll 1
        for (int h = 0; h < kSoloThreads / kPackRows; ++h) {
            const uint64_t b0 = pb + (uint64_t)h * kPackRows;
            const int rows = b0 < A.n_panels ? (int)min<uint64_t>(kPackRows, A.n_panels - b0) : 0;
            pack_tile_rows<kSoloThreads, 4>(A, reinterpret_cast<uint32_t *>(smem), b0, rows);
            if (A.xt) emit_xt_rows<kSoloThreads / 64>(A, reinterpret_cast<const uint32_t *>(smem), b0, rows, lane, wave);
        }
    }
}
