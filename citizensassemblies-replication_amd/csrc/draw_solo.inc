// draw_solo.inc -- the batch LEGACY draw with ONE lane per panel (included by csa_legacy.hip after
// draw_lane.inc; shares its key packing, bcnt_acc, philox_lane, pack_tile_rows and the outcome enum).
//
// Same algorithm and bit-exact output as draw_lane_kernel (legacy.py:47-200, analysis.py:141-159 in
// Philox verification mode), but a lane holds a whole panel's state in registers -- packed
// (need, remaining) for all FN <= 32 features and all WN <= 32 words of the remaining pool -- so a
// wavefront draws 64 panels and nothing is exchanged between lanes in a step.  The two-lane kernel
// runs the holder select, the Philox word choice, the pair exchange and the step control on both
// lanes of a pair; here each runs once per panel.  The price is registers (FN + 2 WN state VGPRs,
// 3 waves per SIMD instead of 4), which the 64 panels per wave more than make up.
//   * find_max_ratio_cat: the lane's FN features in four interleaved chains (features
//     [0, FN/4), [FN/4, FN/2), ...) merged in index order, keeping the first maximum on ties;
//   * holder scan: forward over word pairs (the pair whose preceding holder count is < r is kept),
//     then one compare picks the word and select_bit the agent -- the r-th holder always exists
//     (remaining[f*] is exactly the pool's holder count);
//   * delete_person: packed decrement of all FN keys, "selected == max" from bit-sliced slack planes
//     (FN >= 16) or need < min - max + 1 (FN = 8), as draw_lane_kernel;
//   * cascades (delete_all_in_cat): the cascading lanes (up to kSoloSlots per round) store their new
//     pools in per-wave LDS slots, the 64 lanes recount every feature's remaining (lane = feature,
//     word half) and each owner takes its row of counts;
//   * attempts start on iterations it = 0 mod 4, so every running panel is at step s = it mod 4 and
//     the Philox block of steps s..s+3 (block s/4, oracle/philox.py) is computed every 4th
//     iteration by the whole wave in lockstep; the picks of those 4 steps leave as one 8-byte store.
// The fused pack packs the workgroup's 256 panels in two 128-row tiles.

constexpr int kSoloThreads = 256;
constexpr int kSoloSlots = 8;  // cascading lanes per cooperative round (~3.6 per step and wave at sf_e)

// hh: the household form, which keeps the address ring behind the cascade counts
__host__ __device__ inline size_t solo_lds_bytes(int FN, int WN, int n, bool hh = false) {
    const size_t LS = (size_t)WN + 1;
    const size_t draw = (size_t)FN * LS * 8                            // feature rows
                        + (size_t)((n + 3) & ~3) * 4                  // person feature masks
                        + (size_t)4 * FN * 4                          // need0, rem0, mnx, pad
                        + (size_t)WN * 8                              // attempt-start pool
                        + (size_t)(kSoloThreads / 64) * kSoloSlots * WN * 8   // cascade slots
                        + (size_t)(kSoloThreads / 64) * kSoloSlots * FN * 4   // cascade counts
                        + (hh ? (size_t)((n + 3) & ~3) * 2 : 0);              // address ring (u16)
    const size_t pack = (size_t)kPackRows * (2 * (size_t)WN + 1) * 4;
    return draw > pack ? draw : pack;
}

#ifndef CSA_SOLO_OCC
#define CSA_SOLO_OCC 3
#endif
#ifndef CSA_SOLO_OCC8
#define CSA_SOLO_OCC8 4
#endif

// The two entry points share one function body, draw_solo_body.inc, compiled under each with
// CSA_DRAW_HH = 0 / 1 (HH in the body).  NP: slack bit planes kept (FN >= 16; the instance's largest
// max - selected < 2^NP, as draw_lane_kernel).  HH: the household form (check_same_address,
// legacy.py:78-113): after a pick, every agent of the pick's address ring that is still in the pool is
// deleted unpicked -- its pool bit goes and the remaining half of its features' keys drops by one;
// need, the slack planes and the pick list are untouched -- before the full-feature cascades.  The
// ring is kept as u16[n] in LDS behind the cascade counts.  A mate that an earlier cascade removed is
// no longer in the pool and changes nothing.  The reference's SelectionError inside such a deletion
// (legacy.py:73) is deferred like the others: remaining only falls, so the next step's start test, or
// the need > 0 = remaining classification after the k-th pick, sees the same state.
template <int FN, int WN, int NP, bool K8>
__global__ __launch_bounds__(kSoloThreads, FN <= 8 ? CSA_SOLO_OCC8 : CSA_SOLO_OCC) void draw_solo_kernel(DrawArgs A)
#define CSA_DRAW_HH 0
#include "draw_solo_body.inc"
#undef CSA_DRAW_HH

// the household form (csa_instance_set_address_route CSA_ADDRESS_BATCH): all 8 slack planes
template <int FN, int WN, bool K8>
__global__ __launch_bounds__(kSoloThreads, FN <= 8 ? CSA_SOLO_OCC8 : CSA_SOLO_OCC) void draw_solo_hh_kernel(DrawArgs A)
#define CSA_DRAW_HH 1
#include "draw_solo_body.inc"
#undef CSA_DRAW_HH
