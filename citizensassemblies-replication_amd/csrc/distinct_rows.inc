// distinct_rows.inc -- the distinct rows of a batch of packed panels as a sorted table: rows ascending
// (word 0 most significant, unsigned: np.unique(axis=0)'s order), each with the lowest input index
// holding it and the number of inputs holding it.  Included by csa_legacy.hip inside an anonymous
// namespace, last in the file (kernels are templates of an unused parameter for the reason given in
// multiplicity_exchange.inc's "Layout": every kernel that existed keeps its offset in the code object).
//
// What is sorted is never a row but a record (key, index): `key` is the row's word 0, cached beside the
// index so that most compares are decided without touching the rows, `index` names the row (RsSrc::row).
// rs_less orders records by the whole row and breaks ties by index: a total order, so the unstable
// bitonic network and the merges give one result, and the first record of a run of equal rows is the
// one of lowest index.
//
//   rs_tile_sort_kernel  one workgroup sorts kRsTile records in LDS (bitonic; a partial tile is padded
//                        with sentinel records that order after every row);
//   rs_merge_kernel      one merge pass over pairs of adjacent sorted runs, one output tile of kRsTile
//                        records per workgroup: two lanes find the tile's merge-path diagonals in global
//                        memory, the <= kRsTile records between them go to LDS, every thread finds its own
//                        diagonal there and merges kRsPer records serially;
//   rs_records_kernel    the records of two sorted lists A and B (lengths read on the device), B's run
//                        packed behind A's: one rs_merge_kernel pass over that single pair is the merge;
//   rs_flag_kernel       flag[i] = record i's row differs from record i-1's, and the flags per block;
//   rs_scan_kernel       one workgroup: exclusive scan of the block counts, the list length, the overflow
//                        check against cap_out;
//   rs_pos_kernel        pos[o] = position of the o-th flagged record (pos[D] = n);
//   rs_gather_kernel     out row o = the row of record pos[o]; first / mult from the run
//                        [pos[o], pos[o+1]): in a sort the head's index and the run's length, in a merge
//                        (run length <= 2) the minimum of the firsts and the sum of the mults.
//
// Separate kernels for count, scan and write: no workgroup ever waits for another one's store.
//
// Trip counts.  Every loop is bounded by a host-known size: the binary searches by 33 halvings (lengths
// are below 2^32), row compares by W, serial merges by kRsPer, the scan by the block count of the
// host capacity, merged runs by 2.  Lengths read from the device are clamped to the host capacities
// before use, so no forged length or row makes a loop spin or an index leave its buffer.
constexpr int kRsTile = 1024;   // records per LDS sort / per merge output tile
constexpr int kRsThreads = 256;
constexpr int kRsPer = kRsTile / kRsThreads;
constexpr uint32_t kRsSentinel = 0xFFFFFFFFu;

struct RsSrc {
    const uint64_t *rows_a, *rows_b;      // record index i < split: row i of A, else row i - split of B
    const uint32_t *first_a, *first_b;    // merge only (NULL in a sort: first = index_base + i)
    const uint32_t *mult_a, *mult_b;      // merge only (NULL in a sort: mult = run length)
    uint32_t split;
    int W;
    uint64_t index_base;
    int merged;                           // 0: a sort's records, 1: two lists' records
    __device__ __forceinline__ const uint64_t *row(uint32_t i) const {
        return i < split ? rows_a + (uint64_t)i * W : rows_b + (uint64_t)(i - split) * W;
    }
};

struct RsLen {   // a sort knows n on the host; a merge reads both lengths on the device, clamped
    uint64_t n;
    const unsigned long long *len_a, *len_b;
    uint64_t cap_a, cap_b;
    __device__ __forceinline__ uint64_t a() const { return len_a ? min((uint64_t)*len_a, cap_a) : n; }
    __device__ __forceinline__ uint64_t b() const { return len_a ? min((uint64_t)*len_b, cap_b) : 0; }
    __device__ __forceinline__ uint64_t total() const { return a() + b(); }
};

__device__ __forceinline__ bool rs_less(const RsSrc &s, uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    if (ka != kb) return ka < kb;
    if (ib == kRsSentinel) return ia != kRsSentinel;   // padding orders after every row, key ~0 included
    if (ia == kRsSentinel) return false;
    const uint64_t *ra = s.row(ia), *rb = s.row(ib);
    for (int w = 1; w < s.W; ++w) {
        const uint64_t a = ra[w], b = rb[w];
        if (a != b) return a < b;
    }
    return ia < ib;
}

__device__ __forceinline__ bool rs_same_row(const RsSrc &s, uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    if (ka != kb) return false;
    const uint64_t *ra = s.row(ia), *rb = s.row(ib);
    for (int w = 1; w < s.W; ++w)
        if (ra[w] != rb[w]) return false;
    return true;
}

// merge path: how many of the first d records of merge(A, B) come from A (la + lb < 2^32: 33 halvings)
__device__ __forceinline__ uint32_t rs_merge_path(const RsSrc &s, const uint64_t *ka, const uint32_t *ia, uint32_t la,
                                                  const uint64_t *kb, const uint32_t *ib, uint32_t lb, uint32_t d) {
    uint32_t lo = d > lb ? d - lb : 0u, hi = min(d, la);
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1), j = d - 1 - mid;
        if (rs_less(s, kb[j], ib[j], ka[mid], ia[mid])) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// exclusive scan of one value per thread over the workgroup's kRsThreads threads; *total = their sum
__device__ __forceinline__ uint32_t rs_block_scan(uint32_t v, uint32_t *s_wave, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += up;
    }
    __syncthreads();   // s_wave may still be read from the previous call
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kRsThreads / 64; ++w) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rs_tile_sort_kernel(RsSrc src, uint64_t n, uint64_t *__restrict__ kout,
                                                                  uint32_t *__restrict__ iout) {
    __shared__ uint64_t sk[kRsTile];
    __shared__ uint32_t si[kRsTile];
    const uint64_t base = (uint64_t)blockIdx.x * kRsTile;
    for (int t = threadIdx.x; t < kRsTile; t += kRsThreads) {
        const uint64_t g = base + t;
        const bool in = g < n;
        sk[t] = in ? src.rows_a[g * src.W] : ~0ull;
        si[t] = in ? (uint32_t)g : kRsSentinel;
    }
    __syncthreads();
    for (int k = 2; k <= kRsTile; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < kRsTile / 2; p += kRsThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const uint64_t ki = sk[i], kl = sk[l];
                const uint32_t ii = si[i], il = si[l];
                if (rs_less(src, kl, il, ki, ii) == up) {
                    sk[i] = kl, si[i] = il;
                    sk[l] = ki, si[l] = ii;
                }
            }
            __syncthreads();
        }
    for (int t = threadIdx.x; t < kRsTile; t += kRsThreads) {
        const uint64_t g = base + t;
        if (g < n) {   // the sentinels sorted to the tile's end
            kout[g] = sk[t];
            iout[g] = si[t];
        }
    }
}

// One merge pass.  Sort: runs of L records (L a multiple of kRsTile, so a tile never straddles a pair),
// pair p = runs 2p and 2p+1, the last run possibly short or without partner (then copied).  Merge of two
// lists: the single pair [0, la) and [la, la + lb), lengths from the device.
template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rs_merge_kernel(RsSrc src, RsLen len, uint64_t L,
                                                              const uint64_t *__restrict__ kin,
                                                              const uint32_t *__restrict__ iin,
                                                              uint64_t *__restrict__ kout, uint32_t *__restrict__ iout) {
    __shared__ uint64_t sk[kRsTile];
    __shared__ uint32_t si[kRsTile];
    __shared__ uint32_t s_split[2];
    const uint64_t o = (uint64_t)blockIdx.x * kRsTile;
    uint64_t ps, la, lb;
    if (len.len_a) {
        ps = 0, la = len.a(), lb = len.b();
    } else {
        if (o >= len.n) return;
        ps = o / (2 * L) * (2 * L);
        la = min(L, len.n - ps);
        lb = min(L, len.n - ps - la);
    }
    if (o - ps >= la + lb) return;
    const uint32_t d0 = (uint32_t)(o - ps), d1 = (uint32_t)min((uint64_t)d0 + kRsTile, la + lb);
    const uint64_t *ka = kin + ps, *kb = kin + ps + la;
    const uint32_t *ia = iin + ps, *ib = iin + ps + la;
    if (threadIdx.x < 2)
        s_split[threadIdx.x] = rs_merge_path(src, ka, ia, (uint32_t)la, kb, ib, (uint32_t)lb, threadIdx.x ? d1 : d0);
    __syncthreads();
    const uint32_t a0 = s_split[0], a1 = s_split[1], b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t na = a1 - a0, nb = b1 - b0, m = d1 - d0;   // na + nb == m <= kRsTile
    for (uint32_t t = threadIdx.x; t < m; t += kRsThreads) {
        const bool fa = t < na;
        sk[t] = fa ? ka[a0 + t] : kb[b0 + (t - na)];
        si[t] = fa ? ia[a0 + t] : ib[b0 + (t - na)];
    }
    __syncthreads();
    const uint32_t td = min((uint32_t)threadIdx.x * kRsPer, m);
    uint32_t i = rs_merge_path(src, sk, si, na, sk + na, si + na, nb, td), j = td - i;
    for (int q = 0; q < kRsPer; ++q) {
        if (td + q >= m) break;
        bool take_a = j >= nb;
        if (!take_a && i < na) take_a = !rs_less(src, sk[na + j], si[na + j], sk[i], si[i]);
        const uint32_t from = take_a ? i : na + j;
        kout[ps + d0 + td + q] = sk[from];
        iout[ps + d0 + td + q] = si[from];
        if (take_a) ++i;
        else ++j;
    }
}

// the records of lists A and B, B's run packed behind A's (grid over cap_a + cap_b)
template <int kLate = 0>
__global__ void rs_records_kernel(RsSrc src, RsLen len, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t la = len.a(), lb = len.b();
    if (t < len.cap_a) {
        if (t < la) {
            keys[t] = src.rows_a[t * src.W];
            idx[t] = (uint32_t)t;
        }
    } else if (t - len.cap_a < lb) {
        const uint64_t j = t - len.cap_a;
        keys[la + j] = src.rows_b[j * src.W];
        idx[la + j] = src.split + (uint32_t)j;
    }
}

// flags[i] = record i starts a run of equal rows; bc[block] = flags in the block's kRsTile records
// (grid over the host capacity: blocks past the length write a zero count)
template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rs_flag_kernel(RsSrc src, RsLen len, const uint64_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ idx,
                                                             uint8_t *__restrict__ flags, uint32_t *__restrict__ bc) {
    __shared__ uint32_t s_wave[kRsThreads / 64];
    const uint64_t n = len.total();
    uint32_t c = 0;
    for (int q = 0; q < kRsPer; ++q) {
        const uint64_t i = (uint64_t)blockIdx.x * kRsTile + q * kRsThreads + threadIdx.x;
        if (i < n) {
            const bool head = i == 0 || !rs_same_row(src, keys[i - 1], idx[i - 1], keys[i], idx[i]);
            flags[i] = head ? 1 : 0;
            c += head ? 1u : 0u;
        }
    }
    uint32_t total;
    rs_block_scan(c, s_wave, &total);
    if (threadIdx.x == 0) bc[blockIdx.x] = total;
}

// one workgroup: bc -> exclusive prefix, in place; the list length; pos[D] = n; the overflow check
template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rs_scan_kernel(RsLen len, uint32_t *__restrict__ bc, uint64_t n_blocks,
                                                             uint32_t *__restrict__ pos, uint64_t cap_out,
                                                             unsigned long long *__restrict__ out_len,
                                                             uint32_t *__restrict__ status) {
    __shared__ uint32_t s_wave[kRsThreads / 64];
    uint32_t carry = 0;
    for (uint64_t c0 = 0; c0 < n_blocks; c0 += kRsThreads) {
        const uint64_t b = c0 + threadIdx.x;
        const uint32_t v = b < n_blocks ? bc[b] : 0u;
        uint32_t total;
        const uint32_t ex = rs_block_scan(v, s_wave, &total);
        if (b < n_blocks) bc[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        *out_len = carry;                 // the union's true size, also when it exceeds cap_out
        pos[carry] = (uint32_t)len.total();   // carry <= n: pos holds n + 1 words
        if (carry > cap_out && status) raise_status(status, CSA_E_UNSUPPORTED, 0xFFFFFFFFFFFFFFFFull);
    }
}

template <int kLate = 0>
__global__ __launch_bounds__(kRsThreads) void rs_pos_kernel(RsLen len, const uint8_t *__restrict__ flags,
                                                            const uint32_t *__restrict__ bc, uint32_t *__restrict__ pos) {
    __shared__ uint32_t s_wave[kRsThreads / 64];
    const uint64_t n = len.total();
    const uint64_t i0 = (uint64_t)blockIdx.x * kRsTile + (uint64_t)threadIdx.x * kRsPer;
    uint32_t f[kRsPer], c = 0;
    for (int q = 0; q < kRsPer; ++q) {
        f[q] = i0 + q < n ? flags[i0 + q] : 0u;
        c += f[q];
    }
    uint32_t total;
    uint32_t o = bc[blockIdx.x] + rs_block_scan(c, s_wave, &total);
    for (int q = 0; q < kRsPer; ++q)
        if (f[q]) pos[o++] = (uint32_t)(i0 + q);
}

// out row o (o < min(D, cap_out)) = the row of record pos[o]; grid-stride over the words of the rows
template <int kLate = 0>
__global__ void rs_gather_kernel(RsSrc src, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ pos,
                                 const unsigned long long *__restrict__ out_len, uint64_t cap_out,
                                 uint64_t *__restrict__ out_rows, uint32_t *__restrict__ out_first,
                                 uint32_t *__restrict__ out_mult, uint32_t *__restrict__ status) {
    const uint64_t D = min((uint64_t)*out_len, cap_out), words = D * src.W;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += step) {
        const uint64_t o = t / src.W;
        const int w = (int)(t - o * src.W);
        const uint32_t p0 = pos[o], p1 = pos[o + 1];
        out_rows[t] = src.row(idx[p0])[w];
        if (w) continue;
        if (!src.merged) {   // a sort: ties were broken by index, so the run's head is its lowest index
            if (out_first) out_first[o] = (uint32_t)(src.index_base + idx[p0]);
            if (out_mult) out_mult[o] = p1 - p0;
        } else {             // a merge: a row occurs at most once per list
            uint32_t first = 0xFFFFFFFFu;
            uint64_t mult = 0;
            for (uint32_t p = p0; p < p1 && p < p0 + 2; ++p) {
                const uint32_t r = idx[p];
                const bool in_a = r < src.split;
                first = min(first, in_a ? src.first_a[r] : src.first_b[r - src.split]);
                mult += in_a ? src.mult_a[r] : src.mult_b[r - src.split];
            }
            if (mult > 0xFFFFFFFFull) raise_status(status, CSA_E_UNSUPPORTED, o);
            out_first[o] = first;
            out_mult[o] = (uint32_t)mult;
        }
    }
}

struct RsLayout {   // byte offsets into the scratch of n records
    uint64_t keys[2], idx[2], pos, bc, flags, bytes, n_blocks;
};

__host__ inline RsLayout rs_layout(uint64_t n_records) {
    RsLayout L;
    const uint64_t n = n_records > 1 ? n_records : 1;
    L.n_blocks = (n + kRsTile - 1) / kRsTile;
    L.keys[0] = 0, L.keys[1] = 8 * n;
    L.idx[0] = 16 * n, L.idx[1] = 20 * n;
    L.pos = 24 * n;                          // u32[n + 1]
    L.bc = L.pos + 4 * (n + 1);              // u32[n_blocks]
    L.flags = L.bc + 4 * L.n_blocks;         // u8[n]
    L.bytes = (L.flags + n + 7) & ~7ull;
    return L;
}

// flag, scan, positions, gather over the sorted records (keys, idx): the tail of both operations
__host__ inline int rs_compact(const RsSrc &src, const RsLen &len, uint64_t cap_n, const RsLayout &Y, char *scratch,
                               int buf, uint64_t cap_out, uint64_t *d_out_rows, uint32_t *d_out_first,
                               uint32_t *d_out_mult, uint64_t *d_out_len, uint32_t *d_status, hipStream_t st) {
    const uint64_t *keys = reinterpret_cast<const uint64_t *>(scratch + Y.keys[buf]);
    const uint32_t *idx = reinterpret_cast<const uint32_t *>(scratch + Y.idx[buf]);
    uint32_t *pos = reinterpret_cast<uint32_t *>(scratch + Y.pos), *bc = reinterpret_cast<uint32_t *>(scratch + Y.bc);
    uint8_t *flags = reinterpret_cast<uint8_t *>(scratch + Y.flags);
    unsigned long long *out_len = reinterpret_cast<unsigned long long *>(d_out_len);
    const unsigned nb = (unsigned)Y.n_blocks;
    hipLaunchKernelGGL(rs_flag_kernel<>, dim3(nb), dim3(kRsThreads), 0, st, src, len, keys, idx, flags, bc);
    hipLaunchKernelGGL(rs_scan_kernel<>, dim3(1), dim3(kRsThreads), 0, st, len, bc, Y.n_blocks, pos, cap_out, out_len,
                       d_status);
    hipLaunchKernelGGL(rs_pos_kernel<>, dim3(nb), dim3(kRsThreads), 0, st, len, (const uint8_t *)flags,
                       (const uint32_t *)bc, pos);
    const uint64_t words = std::min(cap_n, cap_out) * (uint64_t)src.W;
    const unsigned grid = (unsigned)std::min<uint64_t>((words + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(rs_gather_kernel<>, dim3(grid ? grid : 1), dim3(256), 0, st, src, idx, (const uint32_t *)pos,
                       (const unsigned long long *)out_len, cap_out, d_out_rows, d_out_first, d_out_mult, d_status);
    return CSA_OK;
}
