// multiplicity_exchange.inc -- the multi-GPU exchange in which the panel multiplicities travel.
// Included by csa_legacy.hip inside an anonymous namespace, as multiplicity.inc is, at the end of the file.
//
// The 24-byte exchange (exchange_keys_kernel / key_unique_kernel / key_verify_kernel) sends one key per
// local distinct panel and the owner counts the distinct panels among them.  Here the key carries the
// rank's count of the panel as a fourth word, and the owner merges instead of counting:
//
//   key = (h1, h2, global index of the panel's first draw on the sender, its multiplicity there)   32 B
//
//   mult_keys_kernel    send side.  The rank's list (csa_unique_mult_async: first, mult, *distinct) is
//                       the local dedupe, so the kernel only buckets it by owner h1 % world into the
//                       fixed-capacity segments, exactly as exchange_keys_kernel does: a per-workgroup
//                       LDS histogram, one global atomic per (workgroup, owner).
//   mkey_insert_kernel  owner, pass 1.  Distinct 128-bit hashes among the valid keys (table: key index
//                       + 1).  The key that takes a slot adds its multiplicity and its index to the
//                       slot's accumulators; a key whose hash equals the slot's resident goes to the
//                       re-draw list as the pair (its panel, the resident's panel) and remembers the slot.
//   (the index-list draw of the listed panels, launch_draw, not counted in the draw statistics)
//   mkey_merge_kernel   owner, pass 2.  A candidate whose re-drawn bitmask equals its resident's is
//                       that panel: it adds into the resident's slot.  One that differs is another
//                       panel behind a 128-bit collision: such candidates are merged among themselves
//                       in a second table keyed by their own bitmask's hash and compared by bitmask,
//                       the way key_verify_kernel counts them.
//   mkey_emit_kernel    both tables' occupied slots -> the list (first, multiplicity), one list_len
//                       atomic per workgroup of 4096 slots; a sum or an index beyond 32 bits fails the
//                       call through the status block.
//
// Layout.  The four kernels are templates (of an unused parameter) so that the compiler emits them where
// it emits the file's template instantiations, in order of first use -- i.e. last: written as plain kernels
// they were laid out ahead of the draw and pair kernels' instantiations, whose offsets in the code object
// then shifted by 0x3600, and bench.py's sf_e step measured 0.2 % slower in four of four alternating runs
// (profiles/dist_mult/).  With them last every kernel that existed keeps its offset.
//
// Accumulators.  acc_m (sum of the multiplicities, zero-filled) and acc_f (lowest global index,
// ~0-filled) are only ever touched by atomicAdd / atomicMin, the slot's winner included: a plain
// store by the winner could land after a later key's atomic and lose it.  Both are 64-bit, so the
// sum cannot wrap before mkey_emit_kernel checks it.  The result is a sum and a minimum: exact and
// deterministic whatever order the keys arrive in; only the list's order is unspecified.
template <int kLate = 0>
__global__ __launch_bounds__(kXbThreads) void mult_keys_kernel(
    const uint64_t *__restrict__ hashes, uint64_t n_panels, const uint32_t *__restrict__ first,
    const uint32_t *__restrict__ mult, const unsigned long long *__restrict__ list_len, uint64_t panel_begin,
    uint32_t world, uint64_t capacity, uint64_t *__restrict__ send_keys,
    unsigned long long *__restrict__ send_counts, uint32_t *__restrict__ status) {
    __shared__ uint32_t hist[kMaxWorld];
    __shared__ unsigned long long rbase[kMaxWorld];
    const uint64_t m = min((uint64_t)*list_len, n_panels);  // entries past the list are never read
    const uint64_t e0 = (uint64_t)blockIdx.x * kXbThreads;
    if (e0 >= m) return;  // whole workgroup
    for (uint32_t w = threadIdx.x; w < world; w += blockDim.x) hist[w] = 0;
    __syncthreads();
    const uint64_t e = e0 + threadIdx.x;
    uint32_t i = 0, owner = 0, local = 0;
    uint64_t h1 = 0, h2 = 0;
    bool valid = e < m;
    if (valid) {
        i = first[e];
        valid = i < n_panels;  // (a list of this batch never holds another index)
    }
    if (valid) {
        h1 = hashes[2 * (uint64_t)i];
        h2 = hashes[2 * (uint64_t)i + 1];
        owner = (uint32_t)(h1 % world);
        local = atomicAdd(&hist[owner], 1u);
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < world; w += blockDim.x)
        rbase[w] = hist[w] ? atomicAdd(&send_counts[w], (unsigned long long)hist[w]) : 0ull;
    __syncthreads();
    if (valid) {
        const uint64_t pos = rbase[owner] + local;
        if (pos < capacity) {
            uint64_t *d = send_keys + 4 * ((uint64_t)owner * capacity + pos);
            d[0] = h1;
            d[1] = h2;
            d[2] = panel_begin + i;
            d[3] = mult[e];
        } else {
            raise_status(status, CSA_E_UNSUPPORTED, kExchangeOverflow);
        }
    }
}

// owner scratch of csa_merge_mult_keys_async, in uint64 words (n = keys, slots = pow2 >= 2n, >= 64):
//   table[slots] acc_m[slots] table2[slots] acc2_m[slots] list_len[1]     zero-filled
//   acc_f[slots] acc2_f[slots]                                           ~0-filled
//   list[2n] cand[2n] rows[2n W]                                          written before they are read
struct MkeyLayout {
    uint64_t slots, zero_words, ones_words, words;
    uint64_t table, acc_m, table2, acc2_m, list_len, acc_f, acc2_f, list, cand, rows;  // word offsets
};

__host__ inline MkeyLayout mkey_layout(uint64_t n_keys, int32_t W) {
    MkeyLayout L;
    const uint64_t n = n_keys > 1 ? n_keys : 1, w = W > 1 ? (uint64_t)W : 1;
    uint64_t slots = 64;
    while (slots < 2 * n) slots <<= 1;
    L.slots = slots;
    L.table = 0, L.acc_m = slots, L.table2 = 2 * slots, L.acc2_m = 3 * slots, L.list_len = 4 * slots;
    L.zero_words = 4 * slots + 1;
    L.acc_f = L.zero_words, L.acc2_f = L.acc_f + slots;
    L.ones_words = 2 * slots;
    L.list = L.acc2_f + slots, L.cand = L.list + 2 * n, L.rows = L.cand + 2 * n;
    L.words = L.rows + 2 * n * w;
    return L;
}

// Owner, pass 1 (keys uint64[total][4]; entry e valid iff e % seg_cap < seg_counts[e / seg_cap]).
// cand[2c] = the candidate's key index, cand[2c + 1] = the slot of the resident whose hash it shares.
template <int kLate = 0>
__global__ void mkey_insert_kernel(const uint64_t *__restrict__ keys, uint64_t total, uint32_t seg_cap,
                                   const uint64_t *__restrict__ seg_counts, unsigned long long *__restrict__ table,
                                   uint64_t mask, unsigned long long *__restrict__ acc_m,
                                   unsigned long long *__restrict__ acc_f, uint64_t *__restrict__ list,
                                   uint64_t *__restrict__ cand, unsigned long long *__restrict__ list_len,
                                   uint64_t list_cap, uint32_t *__restrict__ status) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total || !uq_valid(e, seg_cap, seg_counts)) return;
    const uint64_t h1 = keys[4 * e], h2 = keys[4 * e + 1];
    uint64_t slot = (h1 ^ (h2 >> 29)) & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long v = atomicCAS(table + slot, 0ull, (unsigned long long)(e + 1));
        if (v == 0ull) {  // the slot's winner accumulates like every other key of its panel
            atomicAdd(acc_m + slot, (unsigned long long)keys[4 * e + 3]);
            atomicMin(acc_f + slot, (unsigned long long)keys[4 * e + 2]);
            return;
        }
        const uint64_t j = v - 1;
        if (keys[4 * j] == h1 && keys[4 * j + 1] == h2) {  // same hash: re-draw both to compare
            const unsigned long long c = atomicAdd(list_len, 2ull);
            if (c + 2 <= 2 * list_cap) {
                list[c] = keys[4 * e + 2];
                list[c + 1] = keys[4 * j + 2];
                cand[c] = e;
                cand[c + 1] = slot;
            } else {
                raise_status(status, CSA_E_UNSUPPORTED, kExchangeOverflow);
            }
            return;
        }
        slot = (slot + 1) & mask;
    }
}

// Owner, pass 2 (after the re-draw of the list into rows: candidate c's panel at rows[2c], its
// resident's at rows[2c + 1]).
template <int kLate = 0>
__global__ void mkey_merge_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ rows, int W,
                                  const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ list_len,
                                  uint64_t list_cap, unsigned long long *__restrict__ acc_m,
                                  unsigned long long *__restrict__ acc_f, unsigned long long *__restrict__ table2,
                                  uint64_t mask2, unsigned long long *__restrict__ acc2_m,
                                  unsigned long long *__restrict__ acc2_f) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= list_cap || 2 * c >= *list_len) return;
    const uint64_t e = cand[2 * c];
    const unsigned long long m = keys[4 * e + 3], g = keys[4 * e + 2];
    const uint64_t *x = rows + 2 * c * (uint64_t)W, *y = x + W;
    bool same = true;
    for (int w = 0; w < W && same; ++w) same = x[w] == y[w];
    if (same) {
        const uint64_t slot = cand[2 * c + 1];
        atomicAdd(acc_m + slot, m);
        atomicMin(acc_f + slot, g);
        return;
    }
    uint64_t h1 = 0, h2 = 0;
    for (int w = 0; w < W; ++w) {
        h1 += fmix_a(x[w] ^ ((uint64_t)w * 0x9E3779B97F4A7C15ull));
        h2 += fmix_b(x[w] + ((uint64_t)w + 1) * 0xD6E8FEB86659FD93ull);
    }
    uint64_t slot = (h1 ^ (h2 >> 29)) & mask2;
    for (uint64_t probe = 0; probe <= mask2; ++probe) {
        const unsigned long long v = atomicCAS(table2 + slot, 0ull, (unsigned long long)(c + 1));
        bool here = v == 0ull;
        if (!here) {
            const uint64_t *z = rows + 2 * (v - 1) * (uint64_t)W;
            here = true;
            for (int w = 0; w < W && here; ++w) here = x[w] == z[w];
        }
        if (here) {
            atomicAdd(acc2_m + slot, m);
            atomicMin(acc2_f + slot, g);
            return;
        }
        slot = (slot + 1) & mask2;
    }
}

// The occupied slots of one table -> the list; the kernel runs once per table.  Every thread takes
// kMeSlots consecutive slots and the workgroup reserves its range of the list with ONE atomic (wave scan
// by shuffles, wave totals in LDS): a list_len atomic per wave, as mult_emit_kernel has, is 65 536
// same-address atomics over the 2^22 slots of 1.25 M keys and was 0.4 ms per table.
constexpr int kMeThreads = 1024, kMeSlots = 4;
template <int kLate = 0>
__global__ __launch_bounds__(kMeThreads) void mkey_emit_kernel(const unsigned long long *__restrict__ table,
                                                               const unsigned long long *__restrict__ acc_m,
                                                               const unsigned long long *__restrict__ acc_f,
                                                               uint64_t slots, uint64_t capacity,
                                                               uint32_t *__restrict__ first, uint32_t *__restrict__ mult,
                                                               unsigned long long *__restrict__ out_len,
                                                               uint32_t *__restrict__ status) {
    __shared__ uint32_t wsum[kMeThreads / 64];
    __shared__ unsigned long long base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t t0 = ((uint64_t)blockIdx.x * kMeThreads + threadIdx.x) * kMeSlots;
    uint32_t used = 0, cnt = 0;
    for (int s = 0; s < kMeSlots; ++s)
        if (t0 + s < slots && table[t0 + s] != 0ull) {
            used |= 1u << s;
            ++cnt;
        }
    uint32_t inc = cnt;  // inclusive scan over the wave
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < kMeThreads / 64; ++w) {
            const uint32_t c = wsum[w];
            wsum[w] = tot;
            tot += c;
        }
        base = tot ? atomicAdd(out_len, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    unsigned long long o = base + wsum[wave] + (inc - cnt);
    for (int s = 0; s < kMeSlots; ++s)
        if (used & (1u << s)) {
            const unsigned long long m = acc_m[t0 + s], f = acc_f[t0 + s];
            if (m > 0xFFFFFFFFull || f > 0xFFFFFFFFull) raise_status(status, CSA_E_UNSUPPORTED, kMultOverflow);
            if (o < capacity) {  // (the distinct panels never outnumber the keys)
                first[o] = (uint32_t)f;
                mult[o] = (uint32_t)m;
            }
            ++o;
        }
}
