// multiplicity.inc -- panel multiplicities: how often each distinct panel of a batch was drawn.
// Included by csa_legacy.hip inside its anonymous namespace, after the distinct-panel kernels.
//
// The distinct count (uq_dedupe_kernel, unique_kernel) finds for every entry the table slot of its
// panel and keeps one bit of that.  The kernels here keep the rest: per occupied slot the number of
// entries that landed there (the panel's multiplicity) and the lowest entry index among them (the
// panel's first occurrence), emitted as a list of (first index, multiplicity) pairs, one per distinct
// panel.  The equality rule is the distinct count's: equal 128-bit hashes AND equal W-word bitmasks.
//
//   uq_mult_kernel       the partitioned form, after the unchanged uq_count / uq_scan_part /
//                        uq_scan_tot / uq_scatter passes: one workgroup per partition, two u32 LDS
//                        tables of kUqTable slots (index + 1, multiplicity; 2 x 32 KB, two workgroups
//                        per CU).  The slot's index word is also the first occurrence: inserted by
//                        CAS(0 -> i + 1), lowered by atomicMin on a match -- every value a slot ever
//                        holds names the same panel, so a concurrent comparer that read an older value
//                        still compares against the right rows.
//   unique_mult_kernel   one global table (u64 index + 1) with a u32 counter array beside it, for small
//                        batches, CSA_UNIQUE_PART=0, or a batch beyond the partitioned path;
//   mult_emit_kernel     walks that table and emits the list.
//   mult_spectrum_kernel spectrum[m] = number of listed panels with multiplicity m, plus four summary
//                        words; the list's length is read from the device counter.
//
// The list's order is unspecified (workgroups race for its base); the SET of pairs is exact and
// deterministic, "first" being a minimum.
//
// Same-address adds.  With few distinct panels every copy of a panel meets one slot: 10^6 draws of
// the couples instance are ~10^4 adds per slot.  A lane lowers the index only when its own is below
// the value it just read (the expected number of such lanes is logarithmic in the copies); the count
// is one LDS add per entry.  Counting the matched lanes of a wave per distinct slot with one add
// (ballot / first-lane loop) was built and measured slower on both extremes (DESIGN 4.12,
// profiles/panel_multiplicity_ab/): the skewed batch is bound by one workgroup per panel walking
// ~10^4 entries, as uq_dedupe_kernel is, not by the adds.  mult_spectrum_kernel does aggregate: there
// a batch of distinct panels is 10^6 adds on ONE bin, and the loop runs once per wave.
constexpr int kMsThreads = 256;
constexpr int kMsLdsBins = 8192;   // u32 LDS histogram of mult_spectrum_kernel: n_bins up to here
constexpr int kMsMaxBlocks = 512;

// one add per distinct slot among the wave's lanes with `mine` set (all lanes of the wave call this)
template <typename Ctr>
__device__ __forceinline__ void mult_wave_add(bool mine, uint32_t slot, Ctr *ctr) {
    const int lane = threadIdx.x & 63;
    uint64_t todo = __ballot(mine);
    while (todo) {
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const uint32_t s = (uint32_t)__shfl((int)slot, lead);
        const uint64_t same = __ballot(mine && slot == s);
        if (lane == lead) atomicAdd(ctr + s, (Ctr)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kUqThreads) void uq_mult_kernel(const uint64_t *__restrict__ hashes,
                                                             const uint64_t *__restrict__ panels, int W,
                                                             const uint32_t *__restrict__ idx,
                                                             const uint32_t *__restrict__ base,
                                                             uint32_t *__restrict__ status,
                                                             uint32_t *__restrict__ first,
                                                             uint32_t *__restrict__ mult,
                                                             unsigned long long *__restrict__ list_len) {
    __shared__ uint32_t T[kUqTable];  // lowest entry index + 1 of the slot's panel, 0 = empty
    __shared__ uint32_t M[kUqTable];  // entries of that panel
    __shared__ uint32_t cnt, rbase, rpos;
    for (int t = threadIdx.x; t < kUqTable; t += blockDim.x) {
        T[t] = 0;
        M[t] = 0;
    }
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const uint32_t b0 = base[blockIdx.x], b1 = base[blockIdx.x + 1];
    uint32_t mine = 0;
    for (uint32_t e = b0 + threadIdx.x; e < b1; e += blockDim.x) {
        const uint32_t i = idx[e];
        const uint64_t h1 = hashes[2 * (uint64_t)i], h2 = hashes[2 * (uint64_t)i + 1];
        uint32_t slot = (uint32_t)(h1 ^ (h2 >> 29)) & (kUqTable - 1);
        bool done = false;
        for (int probe = 0; probe < kUqTable && !done; ++probe) {
            const uint32_t v = atomicCAS(&T[slot], 0u, i + 1);
            if (v == 0u) {
                ++mine;
                done = true;
            } else {
                const uint64_t j = v - 1;
                if (hashes[2 * j] == h1 && hashes[2 * j + 1] == h2) {
                    bool same = true;
                    for (int w = 0; w < W && same; ++w) same = panels[(uint64_t)i * W + w] == panels[j * W + w];
                    if (same) {
                        if (i + 1 < v) atomicMin(&T[slot], i + 1);
                        done = true;
                    }
                }
            }
            if (done) atomicAdd(&M[slot], 1u);
            else slot = (slot + 1) & (kUqTable - 1);
        }
        // a full table: more than kUqTable distinct panels in one partition fail the call through
        // the status block, as in uq_dedupe_kernel -- never a short list
        if (!done) raise_status(status, CSA_E_UNSUPPORTED, 0xFFFFFFFFFFFFFFFFull);
    }
    atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) {  // one global atomic per workgroup; the partitions' counts sum to <= n entries
        rbase = cnt ? (uint32_t)atomicAdd(list_len, (unsigned long long)cnt) : 0u;
        rpos = 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kUqTable; t += blockDim.x)
        if (T[t]) {
            const uint32_t o = rbase + atomicAdd(&rpos, 1u);
            first[o] = T[t] - 1u;
            mult[o] = M[t];
        }
}

// one thread per entry: unique_kernel's probing, a counter per slot, atomicMin for the first index
__global__ void unique_mult_kernel(const uint64_t *__restrict__ hashes, const uint64_t *__restrict__ panels,
                                   uint64_t S, int W, unsigned long long *__restrict__ table, uint64_t mask,
                                   uint32_t *__restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    const uint64_t h1 = hashes[2 * i], h2 = hashes[2 * i + 1];
    uint64_t slot = (h1 ^ (h2 >> 29)) & mask;
    for (uint64_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long v = atomicCAS(table + slot, 0ull, (unsigned long long)(i + 1));
        if (v == 0ull) {
            atomicAdd(ctr + slot, 1u);
            return;
        }
        const uint64_t j = v - 1;
        if (hashes[2 * j] == h1 && hashes[2 * j + 1] == h2) {
            bool same = true;
            for (int w = 0; w < W && same; ++w) same = panels[i * W + w] == panels[j * W + w];
            if (same) {
                if (i + 1 < v) atomicMin(table + slot, (unsigned long long)(i + 1));
                atomicAdd(ctr + slot, 1u);
                return;
            }
        }
        slot = (slot + 1) & mask;
    }
}

// the occupied slots of unique_mult_kernel's table -> the list, one list_len atomic per wave
__global__ void mult_emit_kernel(const unsigned long long *__restrict__ table, const uint32_t *__restrict__ ctr,
                                 uint64_t slots, uint32_t *__restrict__ first, uint32_t *__restrict__ mult,
                                 unsigned long long *__restrict__ list_len) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long v = t < slots ? table[t] : 0ull;
    const uint64_t b = __ballot(v != 0ull);
    unsigned long long o = 0;
    if ((threadIdx.x & 63) == 0 && b) o = atomicAdd(list_len, (unsigned long long)__popcll(b));
    o = __shfl(o, 0);
    if (v) {
        o += __popcll(b & ((1ull << (threadIdx.x & 63)) - 1ull));
        first[o] = (uint32_t)(v - 1);
        mult[o] = ctr[t];
    }
}

// spectrum[m] += listed panels with multiplicity m < n_bins; summary = [entries with m >= n_bins, max m,
// sum m^2, sum m].  The list's length comes from *list_len (clamped to capacity); entries past it are
// never read.  Equal multiplicities within a wave go with one add (a batch of distinct panels is one
// bin); use_lds: a per-workgroup u32 histogram (n_bins <= kMsLdsBins), flushed with 64-bit atomics.
__global__ __launch_bounds__(kMsThreads) void mult_spectrum_kernel(const uint32_t *__restrict__ mult,
                                                                   const unsigned long long *__restrict__ list_len,
                                                                   uint64_t capacity,
                                                                   unsigned long long *__restrict__ spectrum,
                                                                   uint64_t n_bins, int use_lds,
                                                                   unsigned long long *__restrict__ summary) {
    __shared__ uint32_t h[kMsLdsBins];
    __shared__ unsigned long long s_sum[4];
    const uint32_t lds_bins = use_lds ? (uint32_t)n_bins : 0u;
    for (uint32_t t = threadIdx.x; t < lds_bins; t += kMsThreads) h[t] = 0;
    if (threadIdx.x < 4) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t len = min((uint64_t)*list_len, capacity);
    const uint64_t step = (uint64_t)gridDim.x * kMsThreads;
    unsigned long long over = 0, mx = 0, sq = 0, sm = 0;
    for (uint64_t e0 = (uint64_t)blockIdx.x * kMsThreads + (threadIdx.x & ~63u); e0 < len; e0 += step) {
        const uint64_t e = e0 + (threadIdx.x & 63);
        const bool valid = e < len;
        const uint32_t m = valid ? mult[e] : 0u;
        if (valid) {
            mx = max(mx, (unsigned long long)m);
            sq += (unsigned long long)m * m;
            sm += m;
            if (m >= n_bins) ++over;
        }
        const bool binned = valid && m < n_bins;
        if (use_lds) mult_wave_add(binned, m, h);
        else mult_wave_add(binned, m, spectrum);
    }
    if (over) atomicAdd(&s_sum[0], over);
    if (mx) atomicMax(&s_sum[1], mx);
    if (sq) atomicAdd(&s_sum[2], sq);
    if (sm) atomicAdd(&s_sum[3], sm);
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < lds_bins; t += kMsThreads)
        if (h[t]) atomicAdd(spectrum + t, (unsigned long long)h[t]);
    if (threadIdx.x == 0) {
        if (s_sum[0]) atomicAdd(summary + 0, s_sum[0]);
        if (s_sum[1]) atomicMax(summary + 1, s_sum[1]);
        if (s_sum[2]) atomicAdd(summary + 2, s_sum[2]);
        if (s_sum[3]) atomicAdd(summary + 3, s_sum[3]);
    }
}
