// draw_dispatch.inc -- the host side of a draw launch (included by csa_legacy.hip inside its anonymous
// namespace, after the draw kernels and the host helpers check_k, reg_kernel_shape, lane_picks and
// launch_pack): the table of built draw kernels, the routing of an instance to one of its rows
// (pick_draw_config), the row's name and launch geometry, and launch_draw, which every entry point
// that draws goes through.

enum class DrawFamily { solo, lane, wide, g16, g64, g64_general };

// One built draw-kernel instantiation (a row of kDrawKernels), and so what pick_draw_config resolves to.
struct DrawConfig {
    DrawFamily family = DrawFamily::g16;
    int fdim = 1, wdim = 1;  // features / pool words per lane: FN / WN of solo and lane, FPL / WPL of the others
    int np = 8;              // solo (FN >= 16) / lane: slack bit planes, csa_instance::max_slack < 2^np
    bool k8 = false;         // solo / lane: the 8-bit need keys carrying their index (csa_instance::need8)
    const void *fn = nullptr;
    bool hh = false;         // solo / lane: the household form (kHouseholdKernels), np = 8
    // lanes that draw one panel together (draw_kernel's and draw_wide_kernel's G)
    int lanes() const {
        switch (family) {
            case DrawFamily::solo: return 1;
            case DrawFamily::lane: return 2;
            case DrawFamily::wide: return 8;
            case DrawFamily::g16: return 16;
            default: return 64;
        }
    }
    bool reg() const { return family == DrawFamily::solo || family == DrawFamily::lane; }  // the register kernels
    bool picks() const { return reg() || family == DrawFamily::wide; }  // pick-list kernels (picks_pack_kernel builds the panels)
};

// holder-scan batch of the lane kernel: all of a lane's row words in one LDS round trip
// (CSA_LANE_SKDIV > 1 splits them, trading a round trip for VGPRs)
#ifndef CSA_LANE_SKDIV
#define CSA_LANE_SKDIV 1
#endif
constexpr int lane_sk(int wn) { return (wn / 2 + CSA_LANE_SKDIV - 1) / CSA_LANE_SKDIV; }

// Every built instantiation, one row each.  A list macro applies X to its leading arguments followed by
// each value of the list, so every family's parameter values stand here once and nowhere else.
#define CSA_KERNEL(...) reinterpret_cast<const void *>(&__VA_ARGS__)
#define CSA_BOTH_K8(X, ...) X(__VA_ARGS__, true) X(__VA_ARGS__, false)
#define CSA_REG_NP(X, ...) X(__VA_ARGS__, 5) X(__VA_ARGS__, 7) X(__VA_ARGS__, 8)  // slack_planes
#define CSA_REG_WN(X) X(4) X(8) X(16) X(28) X(32)
#define CSA_WIDE_WPL(X, ...) X(__VA_ARGS__, 4) X(__VA_ARGS__, 8) X(__VA_ARGS__, 16)
#define CSA_DRAW_FPL(X, ...) X(__VA_ARGS__, 1) X(__VA_ARGS__, 2) X(__VA_ARGS__, 4)
#define CSA_DRAW_WPL64(X, ...) X(__VA_ARGS__, 1) X(__VA_ARGS__, 2) X(__VA_ARGS__, 4)
#define CSA_DRAW_WPL16(X, ...) CSA_DRAW_WPL64(X, __VA_ARGS__) X(__VA_ARGS__, 8) X(__VA_ARGS__, 16)

#define CSA_SOLO_ROW(FN, WN, NP, K8) {DrawFamily::solo, FN, WN, NP, K8, CSA_KERNEL(draw_solo_kernel<FN, WN, NP, K8>)},
#define CSA_SOLO_K8(FN, WN, NP) CSA_BOTH_K8(CSA_SOLO_ROW, FN, WN, NP)
#define CSA_SOLO_FN8(WN) CSA_SOLO_K8(8, WN, 8)  // no slack planes at FN = 8
#define CSA_SOLO_FN16(WN) CSA_REG_NP(CSA_SOLO_K8, 16, WN)
#define CSA_LANE_ROW(FN, WN, NP, K8) \
    {DrawFamily::lane, FN, WN, NP, K8, CSA_KERNEL(draw_lane_kernel<FN, WN, lane_sk(WN), NP, K8>)},
#define CSA_LANE_K8(FN, WN, NP) CSA_BOTH_K8(CSA_LANE_ROW, FN, WN, NP)
#define CSA_LANE_FN32(WN) CSA_REG_NP(CSA_LANE_K8, 32, WN)
#define CSA_WIDE_ROW(FPL, WPL) {DrawFamily::wide, FPL, WPL, 8, false, CSA_KERNEL(draw_wide_kernel<8, FPL, WPL>)},
#define CSA_WIDE_FPL(FPL) CSA_WIDE_WPL(CSA_WIDE_ROW, FPL)
#define CSA_DRAW_ROW(FAMILY, G, GENERAL, FPL, WPL) \
    {DrawFamily::FAMILY, FPL, WPL, 8, false, CSA_KERNEL(draw_kernel<G, FPL, WPL, GENERAL>)},
#define CSA_DRAW_G16(FAMILY, GENERAL, FPL) CSA_DRAW_WPL16(CSA_DRAW_ROW, FAMILY, 16, GENERAL, FPL)
#define CSA_DRAW_G64(FAMILY, GENERAL, FPL) CSA_DRAW_WPL64(CSA_DRAW_ROW, FAMILY, 64, GENERAL, FPL)

const DrawConfig kDrawKernels[] = {
    CSA_REG_WN(CSA_SOLO_FN8) CSA_REG_WN(CSA_SOLO_FN16)
    CSA_REG_WN(CSA_LANE_FN32)
    CSA_WIDE_FPL(2) CSA_WIDE_FPL(4) CSA_WIDE_FPL(5) CSA_WIDE_FPL(8)
    CSA_DRAW_FPL(CSA_DRAW_G16, g16, false)
    CSA_DRAW_FPL(CSA_DRAW_G64, g64, false) CSA_DRAW_FPL(CSA_DRAW_G64, g64_general, true)
};
static_assert(sizeof kDrawKernels / sizeof kDrawKernels[0] == 115, "the set of built draw kernels is fixed");

// The household forms of the register kernels (CSA_ADDRESS_BATCH), a table of their own: every built
// FN / WN / K8 at 8 slack planes, which hold every instance the register kernels take.
#define CSA_SOLO_HH_ROW(FN, WN, K8) \
    {DrawFamily::solo, FN, WN, 8, K8, CSA_KERNEL(draw_solo_hh_kernel<FN, WN, K8>), true},
#define CSA_SOLO_HH8(WN) CSA_BOTH_K8(CSA_SOLO_HH_ROW, 8, WN)
#define CSA_SOLO_HH16(WN) CSA_BOTH_K8(CSA_SOLO_HH_ROW, 16, WN)
#define CSA_LANE_HH_ROW(FN, WN, K8) \
    {DrawFamily::lane, FN, WN, 8, K8, CSA_KERNEL(draw_lane_hh_kernel<FN, WN, lane_sk(WN), K8>), true},
#define CSA_LANE_HH32(WN) CSA_BOTH_K8(CSA_LANE_HH_ROW, 32, WN)

const DrawConfig kHouseholdKernels[] = {CSA_REG_WN(CSA_SOLO_HH8) CSA_REG_WN(CSA_SOLO_HH16) CSA_REG_WN(CSA_LANE_HH32)};
static_assert(sizeof kHouseholdKernels / sizeof kHouseholdKernels[0] == 30, "the set of household kernels is fixed");

// the row with c's family and parameters, into c; false when none is built
bool find_draw_kernel(DrawConfig &c) {
    if (c.hh) {
        for (const DrawConfig &r : kHouseholdKernels)
            if (r.family == c.family && r.fdim == c.fdim && r.wdim == c.wdim && r.k8 == c.k8) {
                c.fn = r.fn;
                return true;
            }
        return false;
    }
    for (const DrawConfig &r : kDrawKernels)
        if (r.family == c.family && r.fdim == c.fdim && r.wdim == c.wdim && r.np == c.np && r.k8 == c.k8) {
            c.fn = r.fn;
            return true;
        }
    return false;
}

// slack bit planes of the register kernels: the built plane counts, the smallest that holds max_slack
int slack_planes(int max_slack) { return max_slack < 32 ? 5 : max_slack < 128 ? 7 : 8; }

// Batch draws: draw_solo_kernel (1 lane per panel) or draw_lane_kernel (2 lanes per panel, 32
// panels per wavefront) when the instance fits -- F <= 32, W <= 32, no max = 0 < min feature, |min|, |selected| < 2^15 (16-bit packed
// need / remaining) and no feature starting above max ("selected == max" is tested as
// need <= min - max) -- else draw_wide_kernel (F <= 64, W <= 128), else draw_kernel with G = 16
// (F <= 64, W <= 256) or 64.  Pick-order / single-attempt draws (general mode) use
// draw_kernel<64, ..., true>.  CSA_DRAW_KERNEL=solo|lane|wide|16|64 forces a batch kernel the instance
// fits (parity tests of every layout).  The family and its bucketed parameters then name one row of
// kDrawKernels (find_draw_kernel).  An instance with address rings draws on draw_kernel<64, ..., true>,
// except a batch draw under CSA_ADDRESS_BATCH of an instance a register kernel takes: that one runs
// the kernel's household form (kHouseholdKernels; CSA_DRAW_KERNEL does not apply).
int pick_draw_config(const csa_instance *I, bool general, DrawConfig &c) {
    const bool reg_ok = I->F <= 32 && I->d_pmask && !I->zero_max_min && I->W <= 32 && I->max_abs < 32768 &&
                        !I->sel_over_max && I->max_slack <= 255;
    const bool lane_ok = reg_ok && I->F > 16;  // built for FN = 32 only
    const bool wide_ok = I->F <= 64 && I->W <= 128 && !I->zero_max_min && I->max_abs < 32768 && !I->sel_over_max;
    const bool g16_ok = I->F <= 64 && I->W <= 256;
    // one lane per panel when a lane holds few features (F <= 16: 142 VGPRs at W = 32, 3 waves/SIMD;
    // example_large_200 281 vs 252 M panels/s, example_small_20 2950 vs 2490); at F = 32 the state needs
    // 165 VGPRs and the two-lane kernel's 4 waves/SIMD win (sf_e 262 vs 247)
    const bool solo_ok = reg_ok && I->F <= 16;
    const bool hh = !general && I->d_addr_next && I->address_route == CSA_ADDRESS_BATCH && (solo_ok || lane_ok);
    general = general || (I->d_addr_next && !hh);  // same-address deletions otherwise: draw_kernel<64, ..., true> only
    using DF = DrawFamily;
    c = DrawConfig();
    c.family = general ? DF::g64_general : solo_ok ? DF::solo : lane_ok ? DF::lane : wide_ok ? DF::wide
               : g16_ok ? DF::g16 : DF::g64;
    const char *e = general || hh ? nullptr : getenv("CSA_DRAW_KERNEL");
    if (e) {
        // the register kernels are built for the shapes they win on only (solo F <= 16, lane F > 16)
        if (!strcmp(e, "solo") && solo_ok) c.family = DF::solo;
        else if (!strcmp(e, "lane") && lane_ok && !solo_ok) c.family = DF::lane;
        else if (!strcmp(e, "wide") && wide_ok) c.family = DF::wide;
        else if (!strcmp(e, "16") && g16_ok) c.family = DF::g16;
        else if (!strcmp(e, "64")) c.family = DF::g64;
    }
    if (c.reg()) {
        reg_kernel_shape(I, c.fdim, c.wdim);
        c.k8 = I->need8;
        c.np = c.fdim >= 16 && !hh ? slack_planes(I->max_slack) : 8;
        c.hh = hh;
    } else if (c.family == DF::wide) {
        const int fpl = (I->F + 7) / 8;
        c.fdim = fpl <= 2 ? 2 : fpl <= 4 ? 4 : fpl <= 5 ? 5 : 8;
        c.wdim = I->W <= 32 ? 4 : I->W <= 64 ? 8 : 16;
    } else {
        c.fdim = pow2_ceil_int((I->F + c.lanes() - 1) / c.lanes());
        c.wdim = pow2_ceil_int(std::max(1, (I->W + c.lanes() - 1) / c.lanes()));
    }
    if (find_draw_kernel(c)) return CSA_OK;
    if (c.picks())
        return fail(CSA_E_UNSUPPORTED, "no %s draw kernel for F=%d W=%d",
                    c.family == DF::solo ? "solo" : c.family == DF::lane ? "lane" : "wide", I->F, I->W);
    return fail(CSA_E_UNSUPPORTED, "no draw kernel for F=%d n=%d (G=%d needs FPL=%d WPL=%d)", I->F, I->n, c.lanes(),
                c.fdim, c.wdim);
}

// The instantiation a DrawConfig stands for, spelled as the profiler prints it (csa_draw_kernel_name,
// csa_draw_kernel_list).
void draw_config_name(const DrawConfig &c, char *buf, size_t len) {
    const char *k8 = c.k8 ? "true" : "false";
    switch (c.family) {
        case DrawFamily::solo:
            if (c.hh) snprintf(buf, len, "draw_solo_hh_kernel<%d, %d, %s>", c.fdim, c.wdim, k8);
            else snprintf(buf, len, "draw_solo_kernel<%d, %d, %d, %s>", c.fdim, c.wdim, c.np, k8);
            break;
        case DrawFamily::lane:
            if (c.hh) snprintf(buf, len, "draw_lane_hh_kernel<%d, %d, %d, %s>", c.fdim, c.wdim, lane_sk(c.wdim), k8);
            else snprintf(buf, len, "draw_lane_kernel<%d, %d, %d, %d, %s>", c.fdim, c.wdim, lane_sk(c.wdim), c.np, k8);
            break;
        case DrawFamily::wide:
            snprintf(buf, len, "draw_wide_kernel<%d, %d, %d>", c.lanes(), c.fdim, c.wdim);
            break;
        default:
            snprintf(buf, len, "draw_kernel<%d, %d, %d, %s>", c.lanes(), c.fdim, c.wdim,
                     c.family == DrawFamily::g64_general ? "true" : "false");
    }
}

// A workgroup of the kernel c at this instance and k: its threads, the panels it draws together and
// its dynamic LDS
struct DrawGeometry {
    int threads, panels_wg;
    size_t lds;
};

DrawGeometry draw_geometry(const DrawConfig &c, const csa_instance *I, int32_t k) {
    DrawGeometry g;
    g.threads = c.family == DrawFamily::lane   ? kLaneThreads
                : c.family == DrawFamily::solo ? kSoloThreads
                : c.family == DrawFamily::wide ? kWideThreads
                                               : draw_threads(c.fdim, c.wdim);
    g.panels_wg = g.threads / c.lanes();
    g.lds = c.family == DrawFamily::lane   ? lane_lds_bytes(c.fdim, c.wdim, I->n, c.hh)
            : c.family == DrawFamily::solo ? solo_lds_bytes(c.fdim, c.wdim, I->n, c.hh)
            : c.family == DrawFamily::wide ? wide_lds_bytes(c.lanes(), c.fdim, c.wdim)
                                           : draw_lds_bytes(c.lanes(), c.fdim, c.wdim, I->W, k, g.panels_wg);
    return g;
}

// workgroups of the kernel c the whole device holds at once: resident workgroups per CU x CUs
int resident_workgroups(const DrawConfig &c, const DrawGeometry &g, int device, uint64_t *out) {
    int per_cu = 0, cus = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, c.fn, g.threads, g.lds));
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    *out = (uint64_t)std::max(per_cu, 1) * (uint64_t)std::max(cus, 1);
    return CSA_OK;
}

// What a caller asks of launch_draw.  `a` is the caller's part of the kernel arguments, copied once:
// k, seed, panel_begin, n_panels, max_attempts (0: the default limit), attempt_base, single, the
// outputs panels / hashes / attempts / picks / status / sel_out / rem_out / present_out, and
//   a.panel_list, a.n_panels_dev: an index-list re-draw (draw_kernel GENERAL; not counted);
//   a.picks16: the pick lists go to this caller buffer and are NOT packed (the caller runs
//     csa_picks_pack_async); otherwise to the instance scratch, packed here into a.panels;
//   a.xt: the register kernels' fused tail also writes XT there when it runs (*xt_written says so).
// launch_draw fills the instance's fields of the arguments itself.
struct DrawRequest {
    DrawArgs a{};
    hipStream_t stream = nullptr;
    int32_t *xt_written = nullptr;
    bool count_stats = true;  // the panels are new ones (csa_instance_draw_stats)
};

int launch_draw(const csa_instance *I, const DrawRequest &rq) {
    DrawArgs A = rq.a;
    const int32_t k = A.k;
    const uint64_t n_panels = A.n_panels;
    const hipStream_t stream = rq.stream;
    uint64_t *const d_panels = A.panels, *const d_hashes = A.hashes;
    uint16_t *const d_picks_ext = A.picks16;
    const bool count_stats = rq.count_stats && !A.panel_list;  // (index-list re-draws are not new panels)
    if (rq.xt_written) *rq.xt_written = 0;
    int rc = check_k(I, k);
    if (rc) return rc;
    if ((!d_panels && !d_picks_ext) || !A.status) return fail(CSA_E_INVALID, "d_panels and d_status are required");
    if (n_panels == 0) return CSA_OK;
    csa_instance *M = const_cast<csa_instance *>(I);  // the draw statistics and the pick-list scratch
    if (k == 0 && !A.single && !A.sel_out && !A.present_out) {
        int rejected = 0;
        for (int f = 0; f < I->F; ++f) rejected |= I->sel0[f] < I->fmin[f];
        // draw statistics as the kernels keep them: accepted new panels only (an index-list re-draw of
        // the multi-GPU owner passes its list capacity as n_panels and draws no new panel)
        if (!rejected && count_stats) M->panels_drawn += n_panels;
        // (a pick-list draw of k = 0 has no panels: nothing to write but the attempts / status)
        if (d_panels) HIPCHK(hipMemsetAsync(d_panels, 0, n_panels * I->W * 8, stream));
        hipLaunchKernelGGL(empty_panels_kernel, dim3((unsigned)((n_panels + 255) / 256)), dim3(256), 0, stream,
                           n_panels, A.attempts, A.status, A.panel_begin, rejected);
        HIPCHK(hipGetLastError());
        if (d_panels && d_hashes) {
            hipLaunchKernelGGL(panel_hash_kernel, dim3((unsigned)((n_panels * 4 + 255) / 256)), dim3(256), 0, stream,
                               d_panels, n_panels, I->W, d_hashes);
            HIPCHK(hipGetLastError());
        }
        return CSA_OK;
    }
    DrawConfig cfg;
    if ((rc = pick_draw_config(I, A.single || A.picks || A.sel_out || A.present_out || A.panel_list, cfg))) return rc;
    A.featmask = I->d_featmask, A.fmin = I->d_fmin, A.fmax = I->d_fmax, A.sel0 = I->d_sel0, A.rem0 = I->d_rem0;
    A.present0 = I->d_present0, A.pmask = I->d_pmask, A.addr_next = I->d_addr_next, A.image = I->d_image;
    A.n = I->n, A.F = I->F, A.W = I->W, A.Ws = I->Ws;
    A.npad = ((I->n + 255) / 256) * 256;  // csa_xt_pad
    if (!A.max_attempts) A.max_attempts = kDefaultMaxAttempts;
    // legacy_find-semantics draws are counted; single attempts (csa_legacy_attempt) are not
    A.stats = (A.single || !count_stats) ? nullptr : I->d_stats;
    if (cfg.reg() && !A.image) return fail(CSA_E_INVALID, "the instance has no draw image");
    if (d_picks_ext && !cfg.picks()) return fail(CSA_E_UNSUPPORTED, "this instance does not take the pick-list draw");
    // (the fused pack's chunked layout reserves whole workgroups of <= 256 panels)
    if (!d_picks_ext && cfg.picks() &&
        (rc = lane_picks(M, ((n_panels + 255) & ~255ull) * (uint64_t)((k + 7) & ~7), stream, &A.picks16)))
        return rc;
    const DrawGeometry g = draw_geometry(cfg, I, k);
    if (g.lds > 160 * 1024) return fail(CSA_E_UNSUPPORTED, "draw kernel needs %zu B of LDS", g.lds);
    // CSA_DRAW_LDS_PAD (diagnostic A/B only): extra bytes of LDS per register-kernel workgroup, to price
    // the occupancy an LDS-resident pick-list tile would cost (128 panels x kpad u16 = 28 KB at sf_e)
    static const size_t lds_pad = [] {
        const char *e = getenv("CSA_DRAW_LDS_PAD");
        return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)0;
    }();
    const size_t lds_launch = cfg.picks() && g.lds + lds_pad <= 160 * 1024 ? g.lds + lds_pad : g.lds;
    // the lane kernel: one workgroup per 128 panels, not persistent -- sf_e 10^6 panels: 4.47 ms vs
    // 5.05 ms for a persistent grid, and retiring workgroups let a concurrent stream's kernels in.
    // draw_kernel: one resident grid (its 66 KB of feature rows at n = 8192 load once per workgroup)
    uint64_t grid = (n_panels + g.panels_wg - 1) / g.panels_wg;
    if (!cfg.picks()) {
        uint64_t resident = 0;
        if ((rc = resident_workgroups(cfg, g, I->device, &resident))) return rc;
        grid = std::min(grid, resident);
    }
    // the lane kernel packs its own panels (one workgroup per 128 panels, so every workgroup knows
    // its panel range); the wide kernel's pick lists are packed by picks_pack_kernel
    const bool fused = cfg.reg() && !d_picks_ext && d_panels;
    if (cfg.reg() && !fused) {
        A.panels = nullptr;
        A.hashes = nullptr;
    }
    if (!fused) A.xt = nullptr;  // only the register kernels' fused tail also writes XT
    if (A.xt && rq.xt_written) *rq.xt_written = 1;
    void *args[] = {&A};
    HIPCHK(hipLaunchKernel(cfg.fn, dim3((unsigned)std::max<uint64_t>(1, grid)), dim3(g.threads), args, lds_launch, stream));
    HIPCHK(hipGetLastError());
    if (!A.single && count_stats) M->panels_drawn += n_panels;
    if (cfg.picks() && !d_picks_ext) {  // pick lists -> packed panels (+ hashes)
        if (!fused && (rc = launch_pack(A.picks16, n_panels, k, I->W, d_panels, d_hashes, stream))) return rc;
        HIPCHK(hipEventRecord(M->picks_done, stream));
        M->picks_pending = true;
    }
    return CSA_OK;
}

// panels one full round of the batch draw's resident workgroups covers (CUs x resident workgroups
// per CU x panels per workgroup): a launch of a multiple of it ends without a part-empty last round
int draw_round_panels(const csa_instance *I, int32_t k, uint64_t *out) {
    *out = 0;
    int rc = check_k(I, k);
    if (rc) return rc;
    DrawConfig cfg;
    if ((rc = pick_draw_config(I, false, cfg))) return rc;
    const DrawGeometry g = draw_geometry(cfg, I, k);
    uint64_t resident = 0;
    if ((rc = resident_workgroups(cfg, g, I->device, &resident))) return rc;
    *out = resident * (uint64_t)g.panels_wg;
    return CSA_OK;
}
