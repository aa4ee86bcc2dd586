// composition.inc -- group_hist_kernel: per-panel group composition (quota and intersection histograms).
// Included by csa_legacy.hip inside its anonymous namespace.
//
// A group is a set of agents as a W-word bitmask in the panels' own encoding.  For every panel p and
// group g the kernel takes c = popcount(panel_p & mask_g) and counts the panel in hist[g][c]: how often
// a quota feature sits on its minimum, how many members of a two-feature intersection a panel holds
// (analysis.py:459-530 can only ask for the mean of that, from the marginals), how often it holds none.
// It is a separate pass over the packed panels every path already holds; no draw kernel is involved.
//
// Shape: lane = group.  A workgroup owns one slab of `slab` consecutive groups (64 while the slab's
// masks fit kGhMaskBytes of LDS, i.e. W <= 128; 32 at W <= 256, ... 1 at W <= 8192) and one range of
// panels.  The slab's masks sit in LDS word-major (s_mask[w][lane]: one ds_read_b64 per word, 512
// contiguous bytes per wave, conflict-free); the panel words are read at a wave-uniform address (the
// wave index goes through readfirstlane, so the loads are scalar loads or a broadcast global load).
// Each wave streams its own panels, two per pass so that one mask read serves both; per panel word
// and lane that is half an LDS read, two ANDs and two bit counts (the compiler unrolls the word loop
// eight times and fetches sixteen dwords per scalar load).  Workgroups of 1024 threads: where the masks
// and the table leave room for one workgroup per CU (n = 8192: 115 KB) sixteen waves share them, not
// eight.  Variants built and measured, none kept: four panels per pass, and the bit count's own addend
// through a register-only asm statement (DESIGN 4.10).  The count goes with one LDS atomic
// add into the lane's own row of a per-workgroup u32[slab][bins | 1] table (odd row stride: the lanes
// of a wave fall on different banks unless their counts differ by the same amount as their rows; lanes
// of one wave never share an entry, waves of the workgroup may, hence the atomic).  At the end the
// non-zero entries go to d_hist with 64-bit global atomic adds.
//
// When masks + table exceed the 160 KB of LDS (bins beyond a few hundred) the table is dropped and each
// count goes straight to d_hist with a global atomic: slow, but every bins >= 1 is served and the
// result is the same table.
//
// A count >= bins is never stored: that lane raises CSA_E_INVALID with the panel index in the status
// block and every other (panel, group) is still counted.  Every d_hist index is (g * bins + c) with
// g < n_groups and c < bins checked at the store.
constexpr int kGhThreads = 1024;          // sixteen waves per workgroup (2.33 -> 1.49 ms at n = 8192, sf_e unchanged)
constexpr int kGhWaves = kGhThreads / 64;
constexpr int kGhMaskBytes = 64 * 1024;   // LDS for one slab's masks: 64 groups up to W = 128
constexpr int kGhMaxW = kGhMaskBytes / 8;  // one group per slab
constexpr int kGhLdsBytes = 160 * 1024;
constexpr int kGhTargetBlocks = 512;       // two workgroups per CU: the flush is per workgroup

__global__ __launch_bounds__(kGhThreads) void group_hist_kernel(const uint64_t *__restrict__ panels,
                                                                uint64_t n_panels, int W,
                                                                const uint64_t *__restrict__ masks, int n_groups,
                                                                int bins, int slab, int use_table,
                                                                unsigned long long *__restrict__ hist,
                                                                uint32_t *__restrict__ status) {
    extern __shared__ uint64_t smem[];
    uint64_t *s_mask = smem;                                                  // [W][slab]
    uint32_t *s_tab = reinterpret_cast<uint32_t *>(smem + (size_t)W * slab);  // [slab][stride]
    const int stride = bins | 1;
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g0 = (int)blockIdx.x * slab;
    const int ng = min(slab, n_groups - g0);

    for (int e = t; e < W * slab; e += kGhThreads) {  // global reads run along a mask's words
        const int j = e / W, w = e - j * W;
        s_mask[w * slab + j] = j < ng ? masks[(size_t)(g0 + j) * W + w] : 0ull;
    }
    if (use_table)
        for (int e = t; e < slab * stride; e += kGhThreads) s_tab[e] = 0u;
    __syncthreads();

    const bool active = lane < ng;
    const int li = active ? lane : 0;  // idle lanes read a valid word and store nothing
    const uint64_t *mrow = s_mask + li;
    unsigned long long *hrow = hist + (size_t)(g0 + li) * (size_t)bins;
    uint32_t *trow = s_tab + (size_t)li * stride;
    const uint64_t step = (uint64_t)gridDim.y * kGhWaves;
    for (uint64_t p0 = (uint64_t)blockIdx.y * kGhWaves + wave; p0 < n_panels; p0 += 2 * step) {
        const uint64_t p1 = p0 + step;
        const bool two = p1 < n_panels;  // wave-uniform
        const uint64_t *a = panels + p0 * (uint64_t)W;
        const uint64_t *b = two ? panels + p1 * (uint64_t)W : a;
        int c0 = 0, c1 = 0;
        for (int w = 0; w < W; ++w) {
            const uint64_t m = mrow[w * slab];
            c0 += __popcll(a[w] & m);
            c1 += __popcll(b[w] & m);
        }
        if (active) {
            if (c0 < bins) {
                if (use_table) atomicAdd(trow + c0, 1u);
                else atomicAdd(hrow + c0, 1ull);
            } else {
                raise_status(status, CSA_E_INVALID, p0);
            }
            if (two) {
                if (c1 < bins) {
                    if (use_table) atomicAdd(trow + c1, 1u);
                    else atomicAdd(hrow + c1, 1ull);
                } else {
                    raise_status(status, CSA_E_INVALID, p1);
                }
            }
        }
    }
    if (!use_table) return;
    __syncthreads();
    for (int e = t; e < slab * stride; e += kGhThreads) {
        const uint32_t v = s_tab[e];
        if (v == 0u) continue;
        const int j = e / stride, c = e - j * stride;
        if (j < ng && c < bins) atomicAdd(hist + (size_t)(g0 + j) * (size_t)bins + c, (unsigned long long)v);
    }
}
