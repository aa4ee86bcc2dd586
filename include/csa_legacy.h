/*
 * csa_legacy.h -- C ABI of the MI355X-native LEGACY Monte Carlo engine
 * (libcsa_legacy.so, built from citizensassemblies-replication_amd/csrc/).
 *
 * The reference (sirandreww/citizensassemblies-replication) has no FFI: its
 * boundary is a Python call surface.  Each entry point below names the
 * reference function it replaces (file:line); the Python mirror in
 * citizensassemblies-replication_amd/{legacy,analysis}.py binds them through
 * ctypes and keeps the reference signatures.  INTEGRATION.md shows the
 * binding a maintainer adds to the reference.
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer; no exception crosses
 *     the ABI; every function returns a CSA_* status code (0 = ok) and leaves
 *     a thread-local message in csa_last_error().
 *   - an instance lives on the HIP device that was current when it was
 *     created.  Multi-GPU: one process per GPU with the RCCL exchange in the
 *     Python layer (DESIGN.md "Multi-GPU"), or several devices of one process
 *     through csa_legacy_sample_devices (replicas owned by the handle).
 *   - agent ids are 0..n-1 = pool row order (analysis.py:131-133); feature
 *     ids are 0..F-1 in category-major CSV order (analysis.py:114-124).
 *   - randomness: Philox4x32-10 verification-mode stream, keyed by
 *     (seed, panel, attempt, step) -- see oracle/philox.py for the contract.
 *   - bitmask panels: uint64 words, W = ceil(n/64) per panel, agent p is
 *     bit (p & 63) of word (p >> 6).
 */
#ifndef CSA_LEGACY_H
#define CSA_LEGACY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------- */
#define CSA_OK 0
#define CSA_E_INVALID 1        /* bad argument / inconsistent instance                         */
#define CSA_E_BAD_QUOTAS 2     /* sum(min) <= k <= sum(max) violated: analysis.py:174-176 assert */
#define CSA_E_NO_CANDIDATE 3   /* no candidate feature: the reference's KeyError, legacy.py:188  */
#define CSA_E_ATTEMPT_LIMIT 4  /* new: the reference restarts forever (analysis.py:146)          */
#define CSA_E_UNSUPPORTED 5    /* instance exceeds the kernels' limits (F > 256, n > 16384, ...) */
#define CSA_E_HIP 6            /* HIP runtime / device error                                     */
#define CSA_E_SELECTION 7      /* one attempt raised SelectionError (legacy.py:34-36)            */

/* ---- flags for csa_legacy_sample ----------------------------------------- */
#define CSA_WANT_PANELS 0x1u   /* copy packed panels (n_panels * W uint64) to panels_out   */
#define CSA_WANT_COUNTS 0x2u   /* per-person counts (analysis.py:179,187)                  */
#define CSA_WANT_PAIRS 0x4u    /* pair co-selection counts (PairHistogram, analysis.py:68) */
#define CSA_WANT_UNIQUE 0x8u   /* number of distinct panels (found_panels, analysis.py:171) */

typedef struct csa_instance csa_instance;

int csa_version(void);                 /* ABI version, currently 1 */
const char *csa_last_error(void);      /* thread-local message of the last failing call */
int csa_device_count(int32_t *out);    /* HIP devices visible to this process */
/* The calling thread's current HIP device (hipGetDevice).  An instance lives on the device that was
 * current at csa_instance_create; the stream-ordered entry points run on the caller's stream, so a
 * caller keeps one instance per device it launches on (the Python layer does: EncodedInstance.handle). */
int csa_current_device(int32_t *out);

/* Encode an instance (replaces read_instance's dicts, analysis.py:108-138).
 * person_feat: n*C global feature ids (row p = agent p, column c = category c);
 * fmin/fmax: F quotas; feat_cat: F category ids (features of one category are
 * contiguous, category-major).  Uploads the feature bitmasks to the current
 * device.  Initial state: selected = 0, remaining = pool counts, all present. */
int csa_instance_create(int32_t n, int32_t C, int32_t F, const int32_t *person_feat,
                        const int32_t *fmin, const int32_t *fmax, const int32_t *feat_cat,
                        csa_instance **out);
void csa_instance_destroy(csa_instance *inst);
/* n, C, F, W = ceil(n/64) */
int csa_instance_info(const csa_instance *inst, int32_t *n, int32_t *C, int32_t *F, int32_t *W);
/* Replace the initial draw state (for find_random_sample_legacy called on
 * partially used dicts): sel/rem: F counters ("selected"/"remaining" of
 * legacy.py's category items), present: W words of the people dict's keys.
 * Any NULL argument restores that part of the default state. */
int csa_instance_set_state(csa_instance *inst, const int32_t *sel, const int32_t *rem,
                           const uint64_t *present);

/* Draw statistics (SURVEY.md section 5 "Metrics"; the reference prints "Rejected" for every
 * min-quota rejection, analysis.py:159, and restarts silently on SelectionError, analysis.py:152-153).
 * Totals over every legacy_find-semantics draw launched on the instance -- csa_legacy_sample,
 * csa_legacy_sample_devices (its per-device replicas included), csa_legacy_find,
 * csa_first_panel_not_in, csa_draw_async / csa_draw_picks_async -- since creation or the last reset
 * (csa_legacy_attempt's single attempts are not counted):
 *   out[0] attempts = accepted panels + out[1] + out[2]
 *   out[1] SelectionError restarts (legacy.py:34-36 raised inside an attempt)
 *   out[2] min-quota rejections (check_min_cats false after k picks, legacy.py:160-168)
 * Synchronises the instance's device(s); reset != 0 zeroes the totals after reading them. */
int csa_instance_draw_stats(csa_instance *inst, int32_t reset, uint64_t *out);
/* Zero the draw statistics without a device-wide synchronisation: with a stream, a memset
 * ordered on it (draws the caller enqueues after it on that stream count from zero); with NULL,
 * after the instance's own streams (csa_legacy_sample's pipeline) are idle.  Other streams of the
 * device are never waited for. */
int csa_instance_draw_stats_reset(csa_instance *inst, void *stream);
/* The same totals as csa_instance_draw_stats (this instance only, not csa_legacy_sample_devices'
 * replicas) written to device memory d_out[0..2] by a kernel on `stream`: no host wait, so a
 * caller orders it after its draws and reads it together with its other results. */
int csa_instance_draw_stats_async(csa_instance *inst, uint64_t *d_out, void *stream);

/* check_same_address (legacy.py:78-99, 103-113): addr_next (n int32) links the agents that share
 * an address (the check_same_address_columns values) into rings, agent order: addr_next[p] = the
 * next agent at p's address, p itself when p lives alone.  With a ring set, every pick deletes
 * the remaining agents at its address (really_delete_person(selected=False)) before the
 * full-category cascades; all draws of the instance then run draw_kernel<64, ..., true>, unless
 * csa_instance_set_address_route says otherwise.
 * NULL removes the rings (the default: the reference harness passes False, analysis.py:150). */
int csa_instance_set_address(csa_instance *inst, const int32_t *addr_next);

/* Where the draws of an instance with address rings run.  CSA_ADDRESS_GENERAL (the default): all of
 * them on draw_kernel<64, ..., true>, one panel per wavefront; csa_draw_xt_async then reports
 * written == 0.  CSA_ADDRESS_BATCH: a batch draw -- no pick order (csa_legacy_find's picks), no single
 * attempt, no state export, no index list -- of an instance that the register kernels take (F <= 32,
 * n <= 2048 and their other conditions, csrc/draw_dispatch.inc) runs the household form of its
 * register kernel, draw_solo_hh_kernel<FN, WN, K8> or draw_lane_hh_kernel<FN, WN, SK, K8>: same
 * panels, attempts and statistics, csa_draw_xt_async reports written == 1, csa_draw_picks_async is
 * offered.  Every other request and every other shape runs as under CSA_ADDRESS_GENERAL.  Without
 * rings the route changes nothing.  An unknown route is CSA_E_INVALID.  csa_legacy_sample_devices
 * copies the route to its replicas. */
#define CSA_ADDRESS_GENERAL 0
#define CSA_ADDRESS_BATCH 1
int csa_instance_set_address_route(csa_instance *inst, int32_t route);

/* ---- host-buffer API (blocking) ------------------------------------------ */

/* legacy_probabilities (analysis.py:162-191) for panels
 * [panel_begin, panel_begin + n_panels): draw every panel with restarts
 * (legacy_find, analysis.py:141-159), then reduce.  Outputs (host memory,
 * each may be NULL when its flag is clear):
 *   panels_out    n_panels * W uint64, panel order            (CSA_WANT_PANELS)
 *   person_counts n int64                                      (CSA_WANT_COUNTS)
 *   pair_counts   n * n int64, row-major; entries i < j and the
 *                 diagonal (= person_counts) are valid; the rest
 *                 is unspecified                               (CSA_WANT_PAIRS)
 *   unique_out    1 uint64 = number of distinct panels          (CSA_WANT_UNIQUE)
 *   attempts_out  n_panels uint32 attempts used per panel (>= 1), or NULL
 * max_attempts caps restarts per panel (0 = default 100000). */
int csa_legacy_sample(csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel_begin,
                      uint64_t n_panels, uint32_t flags, uint32_t max_attempts,
                      uint64_t *panels_out, int64_t *person_counts, int64_t *pair_counts,
                      uint64_t *unique_out, uint32_t *attempts_out);

/* legacy_probabilities (analysis.py:162-191) over several devices of this process: the n_devices
 * argument of SURVEY.md §8(b)'s proposed csa_legacy_sample, for callers without torch.distributed.
 * Shard s (0 <= s < n_shards) draws the contiguous panel range
 *   [panel_begin + n_panels*s/n_shards, panel_begin + n_panels*(s+1)/n_shards)
 * on device devices[s] (NULL: device s; a device may repeat), on a replica of the instance that
 * the handle owns and keeps across calls (it mirrors csa_instance_set_state / _set_address).
 * Per-person and pair counts are summed on shard 0's device (peer copies + an add kernel); every
 * shard reduces its panels to its exact local distinct set and shard 0 counts the union exactly
 * (128-bit hash AND W-word bitmask).  Results are identical to csa_legacy_sample over the same
 * range for any n_shards and device list.  Arguments and outputs as csa_legacy_sample. */
int csa_legacy_sample_devices(csa_instance *inst, const int32_t *devices, int32_t n_shards, int32_t k,
                              uint64_t seed, uint64_t panel_begin, uint64_t n_panels, uint32_t flags,
                              uint32_t max_attempts, uint64_t *panels_out, int64_t *person_counts,
                              int64_t *pair_counts, uint64_t *unique_out, uint32_t *attempts_out);

/* legacy_find (analysis.py:141-159), batched: panels in pick order.
 * picks_out: n_panels * k int32 (a step that picked nobody -- only possible
 * with an inconsistent initial state -- is -1); attempts_out may be NULL. */
int csa_legacy_find(csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel_begin,
                    uint64_t n_panels, uint32_t max_attempts, int32_t *picks_out,
                    uint32_t *attempts_out);

/* One call of find_random_sample_legacy (legacy.py:178-200) = one attempt
 * (seed, panel, attempt) from the instance's initial state.  Returns CSA_OK
 * (picks + final state written), CSA_E_SELECTION (SelectionError; state
 * outputs unspecified) or CSA_E_NO_CANDIDATE.  picks_out: k int32 in pick
 * order, *n_picks set; sel_out/rem_out: F; present_out: W (any may be NULL). */
int csa_legacy_attempt(csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel,
                       uint32_t attempt, int32_t *picks_out, int32_t *n_picks, int32_t *sel_out,
                       int32_t *rem_out, uint64_t *present_out);

/* XMIN's LEGACY caller (_get_panel_not_in_portfolio_if_possible, xmin.py:464-474):
 * draw panels panel_begin, panel_begin+1, ... (at most n_panels; chunks of `chunk`
 * panels, doubling) and stop at the first one that is not in the portfolio (m packed
 * panels, host memory, m*W uint64; exact bitmask comparison behind a device hash
 * table).  *index_out = its offset from panel_begin (-1: all n_panels are members),
 * panel_out (W uint64) = that panel.  A draw error (KeyError / attempt limit) is
 * returned only if every panel before it is a member, as in the reference loop. */
int csa_first_panel_not_in(csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel_begin,
                           uint64_t n_panels, uint32_t max_attempts, const uint64_t *portfolio,
                           uint64_t m, uint64_t chunk, int64_t *index_out, uint64_t *panel_out);

/* MT19937 mode (the reference's own stream), host only, no device
 * needed: `n_panels` consecutive legacy_find calls (analysis.py:141-159; single = 1: ONE
 * find_random_sample_legacy call, legacy.py:178-200, returning CSA_E_SELECTION on a dead end)
 * drawing from the stdlib random stream exactly as legacy.py:149 consumes it.  mt_state: 625
 * uint32 = CPython's random.getstate()[1] (624 words + position), advanced in place.  Instance
 * arrays as csa_instance_create; sel0 / rem0 (F) and present0 (W) give the start state (NULL =
 * 0 / pool counts / everyone), addr_next the same-address rings (or NULL, see
 * csa_instance_set_address).  Outputs (each may be NULL): picks_out n_panels*k (pick order, -1
 * padded), panels_out n_panels*W, attempts_out n_panels; with single, the final sel/rem (F) and
 * remaining pool (W); stats_out (3 uint64) the call's attempts, SelectionErrors and min-quota
 * rejections, as csa_instance_draw_stats counts them (a single attempt that raises counts one
 * SelectionError). */
int csa_legacy_draw_mt(int32_t n, int32_t C, int32_t F, const int32_t *person_feat, const int32_t *fmin,
                       const int32_t *fmax, const int32_t *sel0, const int32_t *rem0, const uint64_t *present0,
                       const int32_t *addr_next, int32_t k, uint32_t *mt_state, uint64_t n_panels,
                       uint32_t max_attempts, int32_t single, int32_t *picks_out, uint64_t *panels_out,
                       uint32_t *attempts_out, int32_t *sel_out, int32_t *rem_out, uint64_t *present_out,
                       uint64_t *stats_out);

/* ---- stream-ordered device API ---------------------------------------------
 * All buffers are device pointers on the instance's device; `stream` is a
 * hipStream_t (NULL = default stream).  Nothing synchronises; errors inside
 * kernels land in d_status (4 uint32: code, panel lo, panel hi, last attempt
 * result) which the caller zeroes before the first launch and decodes with
 * csa_status_decode after synchronising. */

/* Batch draw (analysis.py:141-159 per panel).  The instance's shape picks the kernel: a panel's
 * state (per-feature need / remaining keys and the remaining-pool bitset) lives in REGISTERS, split
 * over 1 lane (draw_solo_kernel, F <= 16), 2 lanes (draw_lane_kernel, F <= 32, n <= 2048) or 8
 * lanes (draw_wide_kernel, F <= 64, n <= 8192) of a wavefront, with the feature rows and person
 * masks in LDS; draw_kernel (16 or 64 lanes per panel) covers every other shape, pick orders and
 * same-address rings.  d_panels: n_panels*W (required); d_hashes: 2*n_panels 128-bit panel hashes
 * (or NULL); d_attempts: n_panels (or NULL); d_picks: n_panels*k (or NULL). */
/* Panels one full round of the batch draw's resident workgroups covers on the instance's device
 * (CUs x resident workgroups per CU x panels per workgroup, for this k): a csa_draw_async launch of
 * a multiple of it ends without a part-empty last round (callers that cut a batch into chunks use
 * it to size them).  *out = 0 on error. */
int csa_draw_round_panels(const csa_instance *inst, int32_t k, uint64_t *out);

int csa_draw_async(const csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel_begin,
                   uint64_t n_panels, uint32_t max_attempts, uint64_t *d_panels,
                   uint64_t *d_hashes, uint32_t *d_attempts, int32_t *d_picks,
                   uint32_t *d_status, void *stream);
/* csa_draw_async that also writes the launch's panels as XT (d_xt: the csa_transpose_count_async
 * layout for n_panels, csa_xt_pad(n) persons per plane) when draw_lane_kernel runs with its fused pack
 * (*xt_written = 1): the caller then skips csa_transpose_count_async and takes the per-person counts
 * from the pair matrix's diagonal (csa_pairs_diag_async).  *xt_written = 0: d_xt untouched, the
 * panels / hashes as csa_draw_async.  flags: CSA_DRAW_RESET_STATUS / CSA_DRAW_RESET_STATS fold a
 * batch's resets into the same call (stream-ordered before the draw).  Replaces the separate transpose pass after one batch's draw
 * (analysis.py:179-190 count the same panels). */
#define CSA_DRAW_RESET_STATUS 0x1u /* csa_draw_xt_async flags: zero d_status (4 words) first, */
#define CSA_DRAW_RESET_STATS 0x2u  /* and this instance's draw statistics, on the stream */
int csa_draw_xt_async(const csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel_begin,
                      uint64_t n_panels, uint32_t max_attempts, uint64_t *d_panels, uint64_t *d_hashes,
                      uint32_t *d_attempts, uint32_t *d_status, uint32_t *d_xt, int32_t *xt_written,
                      uint32_t flags, void *stream);

/* Re-draw panels [panel_begin, panel_begin + n_panels) exactly as csa_draw_async drew them (the same
 * kernel and Philox counters (seed, global panel index, attempt, step), so the same bitmasks), without
 * adding them to the instance's draw statistics.  A sharded run's found_panels (analysis.py:171,186;
 * pickled by run_legacy_or_retrieve, analysis.py:284-290) are re-made this way on whichever rank reads
 * them, instead of being gathered from the other ranks.  d_panels: n_panels*W; d_status as above. */
int csa_redraw_async(const csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel_begin,
                     uint64_t n_panels, uint32_t max_attempts, uint64_t *d_panels, uint32_t *d_status,
                     void *stream);

/* The same draw split in two, for instances whose batch draw is the pick-list kernel
 * (draw_lane_kernel: F <= 32, n <= 2048; csa_draw_picks_supported returns 1 for them, else 0 and
 * csa_draw_picks_async returns CSA_E_UNSUPPORTED).  csa_draw_picks_async writes each panel's k
 * picks in pick order (legacy.py:194 people_selected order) into a row of
 * csa_picks_stride(k) = k rounded up to 8 uint16 (d_picks: n_panels * stride; entries past k
 * unspecified);
 * csa_picks_pack_async turns pick lists into packed panels (n_panels*W) and, if d_hashes is not
 * NULL, their 128-bit hashes.  csa_draw_async = the two back to back on one stream (with an
 * instance-owned pick buffer: concurrent csa_draw_async calls on one instance serialise). */
int32_t csa_picks_stride(int32_t k);
int csa_draw_picks_supported(const csa_instance *inst, int32_t k);
int csa_draw_picks_async(const csa_instance *inst, int32_t k, uint64_t seed, uint64_t panel_begin,
                         uint64_t n_panels, uint32_t max_attempts, uint16_t *d_picks, uint32_t *d_attempts,
                         uint32_t *d_status, void *stream);
int csa_picks_pack_async(const uint16_t *d_picks, uint64_t n_panels, int32_t k, int32_t n, uint64_t *d_panels,
                         uint64_t *d_hashes, void *stream);

/* 128-bit panel hashes (2*n_panels uint64) of packed panels (n_panels*W), the
 * key of the distinct-panel count (replaces hashing the sorted tuples of
 * analysis.py:171,186); identical to the hashes csa_draw_async writes. */
int csa_panel_hash_async(const uint64_t *d_panels, uint64_t n_panels, int32_t W, uint64_t *d_hashes,
                         void *stream);

/* Name of the draw kernel csa_draw_async launches for this instance and k
 * (e.g. "draw_lane_kernel<32, 28, 14, 7, true>"), for matching profiler output; for an instance
 * with address rings the household form where CSA_ADDRESS_BATCH runs it (e.g.
 * "draw_lane_hh_kernel<32, 28, 14, true>"), else the batch kernel's name (never a GENERAL one). */
int csa_draw_kernel_name(const csa_instance *inst, int32_t k, char *buf, uint64_t len);

/* Names of every draw-kernel instantiation the dispatcher can resolve (batch draws and the GENERAL
 * kernels of csa_legacy_find / single attempts / index-list re-draws), newline-separated, spelled as
 * csa_draw_kernel_name spells them: one line per row of the table of built kernels the dispatcher
 * looks its kernel up in (kDrawKernels, csrc/draw_dispatch.inc), in no particular order.  Needs no device.
 * CSA_E_INVALID when buf is NULL or len is too small; csa_last_error then names the size needed. */
int csa_draw_kernel_list(char *buf, uint64_t len);
/* The same for the household forms of the register kernels (CSA_ADDRESS_BATCH), which
 * csa_draw_kernel_list does not name: 30 lines, under the same contract. */
int csa_draw_household_kernel_list(char *buf, uint64_t len);

/* Bit-transpose + per-person count.  Panels (n_panels*W) -> d_xt, the
 * panel-indicator matrix transposed and packed in two 32-bit planes per
 * 64-panel block b (uint32 view): d_xt32[(2b + h) * n_pad + p] holds the bits
 * of agent p for panels 64b + 32h .. 64b + 32h + 31 (bit j = panel
 * 64b + 32h + j); n_pad = csa_xt_pad(n), blocks b < ceil(n_panels/64), i.e.
 * ceil(n_panels/64) * n_pad uint64 of storage.  The planes let the MFMA kernel
 * read every fragment bank-conflict-free.  d_counts (n int64) is ACCUMULATED
 * (+=); d_xt may be NULL (counts only). */
int32_t csa_xt_pad(int32_t n);
int csa_transpose_count_async(const uint64_t *d_panels, uint64_t n_panels, int32_t n,
                              uint64_t *d_xt, int64_t *d_counts, void *stream);

/* Pair counts X^T X on MFMA, upper-triangular 256x256 blocks (replaces
 * PairHistogram.add_portfolio_of_panels_to_histogram,
 * analysis.py:90-95, summed over all panels).  d_xt as produced above
 * (n_blocks = ceil(n_panels/64)); d_pairs (n*n int64, row-major) is
 * ACCUMULATED (+=) for i <= j (lower triangle unspecified).  Exact for any
 * n_blocks (each split stays inside its accumulator's exact integer range).
 * engine: CSA_PAIR_FP4 = v_mfma_scale_f32_32x32x64_f8f6f4 on e2m1 0/1-products
 * (f32 accumulation, exact below 2^24 per split); CSA_PAIR_I8 =
 * v_mfma_i32_32x32x32_i8 (int32 accumulation).  With d_scratch (at least
 * csa_pair_scratch_bytes bytes of device memory) the fp4 engine runs one
 * persistent workgroup per CU with the tiles grouped by XCD (whole tiles stored
 * directly, the leftover tiles as k-pieces summed by a reduce kernel; <= 2^24
 * panels per call, else as below); otherwise each split of the panel blocks
 * writes an int32 partial block that a reduce kernel sums, or, with d_scratch ==
 * NULL, adds into d_pairs with int64 atomics.  csa_pair_counts_async =
 * engine FP4, no scratch.  engine | CSA_PAIR_OVERWRITE stores instead of
 * accumulating: on return d_pairs holds exactly this batch's counts for i <= j
 * (the reduce kernel writes every element of the upper-triangular blocks; without
 * scratch the call zero-fills d_pairs first), so a caller that counts each batch
 * afresh needs no n*n zero-fill of its own.  engine | CSA_PAIR_SHARED is a
 * scheduling hint, never a change of result: the launch will share the CUs with
 * concurrent draw kernels (a pipelined caller).  The library currently takes the
 * same 512-register per-CU form either way (measured faster beside the draws than
 * the 256-register form, which CSA_P2_NB=2 still selects).  engine | CSA_PAIR_ALONE
 * is the opposite hint: nothing runs beside the launch (a serial caller's last
 * batch), so the kernel fastest alone is taken: the per-CU kernel from 2048 panel
 * blocks and 4 tiles per side (n > 768), the split kernel below (measured,
 * profiles/r06_pair_alone/). */
#define CSA_PAIR_FP4 0u
#define CSA_PAIR_I8 1u
#define CSA_PAIR_OVERWRITE 0x100u
#define CSA_PAIR_SHARED 0x200u
#define CSA_PAIR_ALONE 0x400u
uint64_t csa_pair_scratch_bytes(int32_t n, uint64_t n_blocks, uint32_t engine);
int csa_pair_counts_ex_async(const uint64_t *d_xt, uint64_t n_blocks, int32_t n, int64_t *d_pairs,
                             uint32_t engine, void *d_scratch, uint64_t scratch_bytes, void *stream);
int csa_pair_counts_async(const uint64_t *d_xt, uint64_t n_blocks, int32_t n, int64_t *d_pairs,
                          void *stream);

/* Distinct-panel count (found_panels, analysis.py:171,186): two panels are the same iff their
 * 128-bit hashes AND their W-word bitmasks are equal, so the count is exact.  d_panels (n_panels*W)
 * is required.  d_table: table_slots uint64 (power of two >= 2*n_panels) of scratch; *d_unique
 * (uint64) is ACCUMULATED.  With d_status (the 4-word status block) batches of >= 65536 panels take a
 * partitioned path (per-partition LDS tables, no per-panel global atomics); a partition table that
 * overflows sets CSA_E_UNSUPPORTED there.  With d_status == NULL the single global table runs. */
int csa_unique_async(const uint64_t *d_hashes, const uint64_t *d_panels, uint64_t n_panels, int32_t W,
                     uint64_t *d_table, uint64_t table_slots, uint64_t *d_unique, uint32_t *d_status,
                     void *stream);

/* Histogram of the pair counts d_pairs[i][j], i < j (n*n int64, row-major, as
 * produced by csa_pair_counts_*): d_hist[v] (n_bins uint64, zeroed by the call)
 * = number of pairs with count v; pairs with count >= n_bins are counted in
 * *d_overflow (zeroed by the call).  With n_bins = max person count + 1 nothing
 * overflows.  The sorted pair probabilities that
 * plot_pair_probability_distribution_per_algorithm (analysis.py:330-353) draws
 * are v / S repeated d_hist[v] times, v ascending. */
int csa_pair_histogram_async(const int64_t *d_pairs, int32_t n, uint64_t *d_hist, uint64_t n_bins,
                             uint64_t *d_overflow, void *stream);

/* Distinct panels over SEGMENTED input (the owner side of the multi-GPU exchange): n_segments
 * segments of `capacity` entries each (hashes 2*capacity, panels capacity*W uint64 per segment),
 * of which segment s holds d_seg_counts[s] (device uint64) valid leading entries.  Otherwise as
 * csa_unique_async: *d_unique += the exact distinct count; table_slots >= 2*n_segments*capacity. */
int csa_unique_segments_async(const uint64_t *d_hashes, const uint64_t *d_panels, uint32_t n_segments,
                              uint64_t capacity, const uint64_t *d_seg_counts, int32_t W, uint64_t *d_table,
                              uint64_t table_slots, uint64_t *d_unique, uint32_t *d_status, void *stream);

/* Panel multiplicities: the batch as a distribution over whole panels.  For every distinct panel of
 * d_hashes / d_panels (n_panels entries; the equality rule is csa_unique_async's: equal 128-bit hashes
 * AND equal W-word bitmasks) one list entry: d_first[e] = the LOWEST index at which the panel occurs,
 * d_mult[e] = the number of entries that hold it.  d_first / d_mult: n_panels uint32 each; *d_distinct
 * (uint64) is WRITTEN with the list's length (not accumulated).  The order of the list is
 * unspecified and may differ between calls; the set of (first, multiplicity) pairs is exact and
 * deterministic, and the multiplicities sum to n_panels.
 * d_scratch: csa_unique_mult_scratch_bytes(n_panels) bytes (covers both paths below; monotone in
 * n_panels).  Paths as csa_unique_async, the scratch taking the table's place: with d_status, from
 * 65536 entries on and unless CSA_UNIQUE_PART=0, the partitioned pass (per-partition LDS tables);
 * otherwise -- or with d_status == NULL -- one global table.  A partition with more than 8192
 * distinct panels sets CSA_E_UNSUPPORTED in d_status exactly as csa_unique_async does; the list of
 * such a call is not to be used (it is never silently short: the status says so).
 * Stream-ordered, no host wait, nothing allocated.  n_panels == 0 writes *d_distinct = 0 and launches
 * nothing else.  n_panels < 2^32 (CSA_E_UNSUPPORTED above).  CSA_E_INVALID, before any device call,
 * for W < 1, a NULL d_distinct, any other NULL pointer (d_status aside) with n_panels > 0, or
 * scratch_bytes below csa_unique_mult_scratch_bytes(n_panels). */
uint64_t csa_unique_mult_scratch_bytes(uint64_t n_panels);
int csa_unique_mult_async(const uint64_t *d_hashes, const uint64_t *d_panels, uint64_t n_panels, int32_t W,
                          void *d_scratch, uint64_t scratch_bytes, uint32_t *d_first, uint32_t *d_mult,
                          uint64_t *d_distinct, uint32_t *d_status, void *stream);

/* Multiplicity spectrum of a list csa_unique_mult_async wrote: d_spectrum[m] (n_bins uint64, zeroed
 * by the call) = number of list entries with multiplicity m < n_bins, over the first
 * min(*d_distinct, capacity) entries of d_mult -- the length is read on the device, entries past it
 * are never read.  d_summary (4 uint64, zeroed by the call): [0] entries with multiplicity >= n_bins
 * (not in the spectrum), [1] the largest multiplicity, [2] the sum of the squared multiplicities,
 * [3] the sum of the multiplicities -- which equals the number of entries the list was made from and
 * is the pass's self-check.  With n_bins = [1] + 1 nothing overflows.  Every n_bins >= 1 is served
 * (a per-workgroup LDS histogram up to 8192 bins, straight to d_spectrum above).  Stream-ordered, no
 * host wait.  CSA_E_INVALID, before any device call, for n_bins < 1 or a NULL pointer (d_mult may be
 * NULL with capacity == 0). */
int csa_mult_spectrum_async(const uint32_t *d_mult, const uint64_t *d_distinct, uint64_t capacity,
                            uint64_t *d_spectrum, uint64_t n_bins, uint64_t *d_summary, void *stream);

/* Multi-GPU distinct-panel exchange, send side (no host synchronisation; replaces the reference's
 * per-run `found_panels` set, analysis.py:171,186, across ranks).  The exact LOCAL distinct panels
 * of d_hashes / d_panels (n_panels, hash AND bitmask equality) are bucketed by owner rank
 * h1 % world into fixed-capacity segments: d_send_hashes uint64[world][capacity][2],
 * d_send_panels uint64[world][capacity][W], d_send_counts uint64[world] (entries per segment;
 * unused entries are left unwritten).  All three feed equal-split all_to_alls; the owner then calls
 * csa_unique_segments_async on what it received.  A segment that would exceed `capacity` raises
 * CSA_E_UNSUPPORTED in d_status (required).  d_scratch: csa_exchange_scratch_bytes(n_panels) bytes.
 * world <= 1024, n_panels < 2^31. */
uint64_t csa_exchange_scratch_bytes(uint64_t n_panels);
int csa_exchange_pack_async(const uint64_t *d_hashes, const uint64_t *d_panels, uint64_t n_panels, int32_t W,
                            uint32_t world, uint64_t capacity, void *d_scratch, uint64_t scratch_bytes,
                            uint64_t *d_send_hashes, uint64_t *d_send_panels, uint64_t *d_send_counts,
                            uint32_t *d_status, void *stream);

/* The 24-byte distinct-panel exchange.  A panel is a pure function of (seed, global panel index) in
 * the Philox stream, so instead of its bitmask each local distinct panel travels as a key
 * (h1, h2, panel_begin + local index).  Send side (as csa_exchange_pack_async otherwise):
 * d_send_keys uint64[world][capacity][3], scratch csa_exchange_scratch_bytes(n_panels).  Owner
 * side: *d_unique += the exact number of distinct panels among the valid keys of n_segments
 * segments of `capacity` keys (segment s holds d_seg_counts[s]): the distinct 128-bit hashes, plus
 * -- every key whose hash matched an earlier key being re-drawn on inst (draw over an index list,
 * Philox (k, seed, max_attempts) as the original draws) together with that key's panel -- the
 * mismatched ones (128-bit hash collisions) counted exactly by bitmask.  d_scratch:
 * csa_unique_keys_scratch_bytes(n_segments * capacity, W) bytes. */
int csa_exchange_keys_async(const uint64_t *d_hashes, const uint64_t *d_panels, uint64_t n_panels, int32_t W,
                            uint64_t panel_begin, uint32_t world, uint64_t capacity, void *d_scratch,
                            uint64_t scratch_bytes, uint64_t *d_send_keys, uint64_t *d_send_counts,
                            uint32_t *d_status, void *stream);
uint64_t csa_unique_keys_scratch_bytes(uint64_t n_keys, int32_t W);
int csa_unique_keys_async(const csa_instance *inst, int32_t k, uint64_t seed, uint32_t max_attempts,
                          const uint64_t *d_keys, uint32_t n_segments, uint64_t capacity,
                          const uint64_t *d_seg_counts, void *d_scratch, uint64_t scratch_bytes,
                          uint64_t *d_unique, uint32_t *d_status, void *stream);

/* The 32-byte exchange: the panel multiplicities of a sharded run.  The key of the 24-byte exchange
 * with the rank's count of the panel as a fourth word, (h1, h2, panel_begin + first, multiplicity),
 * merged -- not counted -- by the owner.
 *
 * Send side: the list csa_unique_mult_async wrote over this rank's d_hashes (n_panels entries):
 * d_first / d_mult, of which the first min(*d_distinct, n_panels) entries are read -- the length on
 * the device, entries past it never.  Every listed panel becomes one key in d_send_keys
 * uint64[world][capacity][4], bucketed by owner h1 % world; d_send_counts uint64[world] (zeroed by the
 * call) = keys per segment, unused keys are left unwritten.  The list IS the local dedupe: the call
 * runs none of its own and needs no scratch.  A segment that would exceed `capacity` raises
 * CSA_E_UNSUPPORTED in d_status (required), never a short segment.  n_panels == 0 writes zero counts
 * and launches nothing else.  world <= 1024; panel_begin + n_panels <= 2^32 (CSA_E_UNSUPPORTED
 * above: the merged list's indices are uint32).  CSA_E_INVALID, before any device call, for world or
 * capacity == 0, a NULL d_send_keys / d_send_counts / d_status / d_distinct, or any other NULL
 * pointer with n_panels > 0.
 *
 * Owner side: over the valid keys of n_segments segments of `capacity` keys (segment s holds
 * d_seg_counts[s], device uint64) one list entry per distinct panel: d_mult[e] = the sum of its keys'
 * multiplicities, d_first[e] = the lowest of their global indices.  d_first / d_mult: n_segments *
 * capacity uint32 each, entries past the list hold zero; *d_distinct (uint64) is WRITTEN with the
 * list's length (not accumulated).  Equality is csa_unique_async's, equal 128-bit hash AND equal
 * bitmask: every key whose hash matches an earlier key is re-drawn on inst together with that key's
 * panel (draw over an index list, Philox (k, seed, max_attempts) as the original draws, not counted
 * in the draw statistics); equal bitmasks merge, a key behind a 128-bit collision gets an entry of its
 * own, such keys merged among themselves by bitmask.  The order of the list is unspecified; the set of
 * (first, multiplicity) pairs is exact and deterministic.  A merged multiplicity or index beyond
 * uint32 raises CSA_E_UNSUPPORTED in d_status (required); n_segments * capacity < 2^32
 * (CSA_E_UNSUPPORTED above).  d_scratch: csa_merge_mult_keys_scratch_bytes(n_segments * capacity, W)
 * bytes.  Stream-ordered, no host wait, nothing allocated.  CSA_E_INVALID, before any device call,
 * for a NULL pointer, capacity == 0, n_segments == 0 or scratch_bytes below that size. */
int csa_exchange_mult_keys_async(const uint64_t *d_hashes, uint64_t n_panels, const uint32_t *d_first,
                                 const uint32_t *d_mult, const uint64_t *d_distinct, uint64_t panel_begin,
                                 uint32_t world, uint64_t capacity, uint64_t *d_send_keys,
                                 uint64_t *d_send_counts, uint32_t *d_status, void *stream);
uint64_t csa_merge_mult_keys_scratch_bytes(uint64_t n_keys, int32_t W);
int csa_merge_mult_keys_async(const csa_instance *inst, int32_t k, uint64_t seed, uint32_t max_attempts,
                              const uint64_t *d_keys, uint32_t n_segments, uint64_t capacity,
                              const uint64_t *d_seg_counts, void *d_scratch, uint64_t scratch_bytes,
                              uint32_t *d_first, uint32_t *d_mult, uint64_t *d_distinct, uint32_t *d_status,
                              void *stream);

/* The distinct panels as a sorted table (reading the reference's `found_panels` set, analysis.py:171,
 * 186, and what it pickles, analysis.py:290, without a host copy of all S panels).  Rows are W uint64
 * words, row-major (the panels' own layout); their order is lexicographic with word 0 most significant,
 * every word compared unsigned -- np.unique(axis=0)'s order, PanelSet.rows()'s.  Both operations are
 * stream-ordered, read lengths on the device, wait for nothing and allocate nothing.
 *
 * Sort-unique of a chunk: d_out_rows (n_rows * W words) receives the distinct rows of d_rows ascending;
 * per output row d_first (or NULL) = index_base + the lowest input index holding it, d_mult (or NULL) =
 * the number of input rows holding it (n_rows uint32 each); *d_distinct (uint64) is WRITTEN with the
 * list's length.  Output entries past the length are unspecified; nothing outside the stated sizes is
 * written and d_rows is not modified.  An LDS sort of csa_rows_sort_tile() records (word 0, index) per
 * workgroup, merge passes over pairs of runs partitioned by merge path, then flag / scan / gather.
 * d_scratch: csa_rows_sort_scratch_bytes(n_rows, W) bytes, 8-byte aligned.  n_rows == 0 writes
 * *d_distinct = 0 and launches nothing else.  d_status is not used by the sort (may be NULL).
 * CSA_E_UNSUPPORTED for index_base + n_rows > 2^32 (d_first is uint32, as in the merged multiplicity
 * lists) and for n_rows == 2^32.  CSA_E_INVALID, before any device call, for W < 1, a NULL d_distinct,
 * a NULL d_rows / d_scratch / d_out_rows with n_rows > 0, scratch_bytes below the stated size, or
 * d_out_rows overlapping d_rows.
 *
 * Merge-unique of two such lists: A and B, each sorted and distinct with its first and mult, lengths
 * min(*d_a_len, cap_a) and min(*d_b_len, cap_b) read on the device -- entries past a length are never
 * read.  The output is the sorted distinct union; a row present in both gets first = min(first_A,
 * first_B) and mult = mult_A + mult_B.  *d_out_len (uint64) is WRITTEN with the union's size.  A union
 * larger than cap_out sets CSA_E_UNSUPPORTED in d_status (required) and writes nothing past cap_out
 * rows (*d_out_len still holds the union's size); so does a merged mult beyond uint32.  The sort's
 * merge-path pass and compaction, over one pair of runs.  d_scratch:
 * csa_rows_merge_scratch_bytes(cap_a, cap_b, W) bytes, 8-byte aligned.  cap_a + cap_b == 0 writes
 * *d_out_len = 0 and launches nothing else.  CSA_E_UNSUPPORTED for cap_a + cap_b >= 2^32 - 1.
 * CSA_E_INVALID, before any device call, for W < 1, a NULL length pointer or d_status, a NULL list
 * pointer with a non-zero capacity, a NULL output or scratch with work to do, scratch_bytes below the
 * stated size, d_out_rows overlapping an input list, or d_out_len being one of the input lengths. */
int32_t csa_rows_sort_tile(void);
uint64_t csa_rows_sort_scratch_bytes(uint64_t n_rows, int32_t W);
int csa_rows_sort_unique_async(const uint64_t *d_rows, uint64_t n_rows, int32_t W, uint64_t index_base,
                               void *d_scratch, uint64_t scratch_bytes, uint64_t *d_out_rows,
                               uint32_t *d_first /* or NULL */, uint32_t *d_mult /* or NULL */,
                               uint64_t *d_distinct, uint32_t *d_status, void *stream);
uint64_t csa_rows_merge_scratch_bytes(uint64_t cap_a, uint64_t cap_b, int32_t W);
int csa_rows_merge_unique_async(const uint64_t *d_a_rows, const uint32_t *d_a_first, const uint32_t *d_a_mult,
                                const uint64_t *d_a_len, uint64_t cap_a, const uint64_t *d_b_rows,
                                const uint32_t *d_b_first, const uint32_t *d_b_mult, const uint64_t *d_b_len,
                                uint64_t cap_b, int32_t W, void *d_scratch, uint64_t scratch_bytes,
                                uint64_t *d_out_rows, uint32_t *d_out_first, uint32_t *d_out_mult,
                                uint64_t cap_out, uint64_t *d_out_len, uint32_t *d_status, void *stream);

/* Two such tables side by side (the reference draws LEGACY twice, seeds 0 and 1, and reads one sample's
 * result in the other, analysis.py:536-541; it prints found_panels beside LEXIMIN's and XMIN's sets,
 * analysis.py:575-582): the join of two tables and the lookup of a few rows in one.  Both are
 * stream-ordered, read lengths on the device, wait for nothing and allocate nothing.
 *
 * Join: A and B in the merge's input form -- rows sorted and distinct, lengths min(*d_a_len, cap_a) and
 * min(*d_b_len, cap_b) read on the device, entries past a length never read; d_a_mult / d_b_mult uint32
 * per row, or NULL: every multiplicity of that table is 1.  Every row of the sorted distinct union has a
 * class: 1 = only in A, 2 = only in B, 4 = in both.  The union rows whose class is in the mask `select`
 * go, ascending, to d_out_rows (cap_out * W words), with d_out_mult_a / d_out_mult_b (cap_out uint32
 * each) = the row's multiplicity on that side, 0 where it is absent; each of the three may be NULL, and
 * all are ignored with select == 0.  *d_out_len (uint64) is WRITTEN with the number of selected rows; a
 * number beyond cap_out sets CSA_E_UNSUPPORTED in d_status (required) and writes nothing past cap_out
 * rows.  d_record (11 uint64, required) is WRITTEN with the summary of the whole union, whatever select:
 *   [0] union size            [1] rows in both          [2] rows only in A      [3] rows only in B
 *   [4] sum of mult_a over A  [5] sum of mult_b over B  [6] sum of mult_a over the rows in both
 *   [7] sum of mult_b over the rows in both             [8] sum of mult_a * mult_b over the rows in both
 *   [9] sum of min(mult_a * scale_b, mult_b * scale_a) over the rows in both
 *   [10] 1 if a sum did not fit 64 bits (only [8] and [9] can fail to), else 0; 1 also sets
 *        CSA_E_UNSUPPORTED in d_status, and [8] / [9] then hold the low 64 bits.
 * With scale_a = sum of A's mults and scale_b = sum of B's, [9] / (scale_a * scale_b) is the overlap
 * sum min(p_A, p_B) of the two empirical distributions and [8] / (scale_a * scale_b) the cross-sample
 * estimate of the sum of squared probabilities.  Every sum is an exact integer, the same on every run:
 * integer adds only, carried in 128 bits where 64 can overflow; no float arithmetic, no atomics.  The
 * merge's record and merge-path passes over the one pair of runs, then the join's own flag / scan /
 * summary / position / gather.  d_scratch: csa_rows_join_scratch_bytes(cap_a, cap_b, W) bytes, 8-byte
 * aligned.  cap_a + cap_b == 0 writes *d_out_len = 0 and a zero record and launches nothing else.
 * CSA_E_UNSUPPORTED for cap_a + cap_b >= 2^32 - 1.  CSA_E_INVALID, before any device call, for W < 1, a
 * NULL length, d_out_len, d_record or d_status, NULL rows with a non-zero capacity, a NULL scratch with
 * work to do, scratch_bytes below the stated size, select > 7, a scale >= 2^32, an output overlapping an
 * input list, or d_out_len / d_record overlapping a length.
 *
 * Lookup: d_out_index[q] (uint32) = the index of the row of the table (d_rows, min(*d_len, cap) rows)
 * equal to query row q of d_queries (n_queries * W words), or 0xFFFFFFFF.  Queries need be neither
 * sorted nor distinct; one binary search of at most 33 halvings each; no scratch.  n_queries == 0
 * launches nothing.  CSA_E_UNSUPPORTED for cap >= 2^32 - 1.  CSA_E_INVALID, before any device call, for
 * W < 1, a NULL d_len, NULL rows with a non-zero capacity, NULL queries or output with n_queries > 0,
 * or d_out_index overlapping an input. */
uint64_t csa_rows_join_scratch_bytes(uint64_t cap_a, uint64_t cap_b, int32_t W);
int csa_rows_join_async(const uint64_t *d_a_rows, const uint32_t *d_a_mult /* or NULL */, const uint64_t *d_a_len,
                        uint64_t cap_a, const uint64_t *d_b_rows, const uint32_t *d_b_mult /* or NULL */,
                        const uint64_t *d_b_len, uint64_t cap_b, int32_t W, uint32_t select, uint64_t scale_a,
                        uint64_t scale_b, void *d_scratch, uint64_t scratch_bytes,
                        uint64_t *d_out_rows /* or NULL */, uint32_t *d_out_mult_a /* or NULL */,
                        uint32_t *d_out_mult_b /* or NULL */, uint64_t cap_out, uint64_t *d_out_len,
                        uint64_t *d_record, uint32_t *d_status, void *stream);
int csa_rows_find_async(const uint64_t *d_rows, const uint64_t *d_len, uint64_t cap, int32_t W,
                        const uint64_t *d_queries, uint64_t n_queries, uint32_t *d_out_index, void *stream);

/* A weight per agent against a table of panels: which row has the largest weight sum?  Both loops of the
 * reference's column generation put that question to an ILP over all feasible panels -- the
 * multiplicative-weights stage of _generate_initial_committees (xmin.py:229-290, leximin.py:236-300) 3 n
 * times, the inner loop of _expand_distribution_leximin (xmin.py:410-440) once per LP iteration with the
 * dual values.  These entry points answer it over panels that were DRAWN (a run's table of distinct panels,
 * or chunks of fresh draws): heuristic pricing, no ILP and no LP.  All are stream-ordered, read the length
 * on the device, wait for nothing and allocate nothing.
 *
 * Table: d_rows uint64[cap][W] in the tables' row form (agent p = bit p & 63 of word p >> 6, padding bits
 * zero), min(*d_len, cap) valid rows; a row past the length is never read.  n agents, 0 < n <= 64 * W.
 * d_weights: n float64.
 *
 * Price: score of row d = the sum of d_weights[i] over the set bits i of row d, in float64, starting from
 * +0.0 with one rounded add per member in ASCENDING agent index (no reassociation: a host loop gives the
 * same bits).  d_scores (cap float64, or NULL) receives the scores of the valid rows; entries past the
 * length are not written.  d_best (2 uint64, required) receives index_base + the best row and its score's
 * bits: scores compare as float64 values with >, ties go to the lowest row.  An empty table gives
 * CSA_PRICE_NONE and -inf.  With CSA_PRICE_ACCUMULATE in flags the stored d_best is replaced only by a
 * strictly greater score, or when it holds CSA_PRICE_NONE (an empty table then leaves it as it is): chunks
 * priced in ascending index order keep the lowest global index among ties, whatever the chunk size.
 * d_scratch: csa_rows_price_scratch_bytes(cap, W) bytes, 8-byte aligned (one (row, score) per
 * csa_rows_price_tile() rows).
 *
 * MW cover: `rounds` rounds of the multiplicative-weights stage over the table, each a price pass and one
 * workgroup's update, 2 * rounds plain launches with no host wait between them.  Round r: p = the best row
 * under d_weights; d_picks[r] = p (uint32); d_pick_scores[r] (or NULL) = its score; w[i] *= 0.8 for the
 * members of row p; s = the lane-strided sum of w (partial[l] = sum over ascending j of w[64 j + l] from
 * +0.0 over the array padded with +0.0 to 64 * W entries, then s = the sum over ascending l of partial[l]
 * from +0.0); f = n / s; w[i] *= f for all i; then if d_chosen[p] (uint8 per row) was set, w[i] = 0.9 *
 * w[i] + 0.1 for all i with the product and the sum rounded separately, else d_chosen[p] = 1 -- the order
 * of xmin.py:251-266.  d_weights and d_chosen are read and written, so a second call continues the first.
 * An empty table leaves the weights alone and writes 0xFFFFFFFF picks (and -inf pick scores).  rounds == 0
 * launches nothing.  The scratch is the price pass's.
 *
 * First holder: d_first_row[i] (n uint32) = the lowest valid row whose bit i is set, or 0xFFFFFFFF.
 *
 * CSA_E_UNSUPPORTED for cap >= 2^32 - 1 or a W whose weights exceed the LDS.  CSA_E_INVALID, before any
 * device call, for W < 1, n <= 0, n > 64 * W, a NULL d_len, NULL rows with a non-zero capacity, a NULL
 * weights / d_best / d_chosen / d_picks / d_first_row where one is needed, unknown flags, a scratch that is
 * NULL, short or misaligned with cap > 0, or an output overlapping the table or its length. */
#define CSA_PRICE_ACCUMULATE 0x1u
#define CSA_PRICE_NONE 0xFFFFFFFFFFFFFFFFull
uint64_t csa_rows_price_tile(void);
uint64_t csa_rows_price_scratch_bytes(uint64_t cap, int32_t W);
int csa_rows_price_async(const uint64_t *d_rows, const uint64_t *d_len, uint64_t cap, int32_t W, int32_t n,
                         const double *d_weights, uint64_t index_base, uint32_t flags, double *d_scores /* or NULL */,
                         uint64_t *d_best, void *d_scratch, uint64_t scratch_bytes, void *stream);
int csa_rows_mw_cover_async(const uint64_t *d_rows, const uint64_t *d_len, uint64_t cap, int32_t W, int32_t n,
                            uint32_t rounds, double *d_weights, uint8_t *d_chosen, uint32_t *d_picks,
                            double *d_pick_scores /* or NULL */, void *d_scratch, uint64_t scratch_bytes,
                            void *stream);
int csa_rows_first_holder_async(const uint64_t *d_rows, const uint64_t *d_len, uint64_t cap, int32_t W, int32_t n,
                                uint32_t *d_first_row, void *stream);

/* The maximin lottery over a table of drawn panels: the reference's _dual_leximin_stage with no fixed
 * probabilities and P ranging over the table's rows (xmin.py:293-321, the first outer iteration of
 * _expand_distribution_leximin) --
 *     maximise z  s.t.  sum over the rows P holding i of x_P >= z for every agent i some row holds,
 *                       sum of x_P = 1,  x >= 0
 * -- solved as a zero-sum game by the multiplicative-weights loop, no LP solver.  After T rounds x = (how often
 * each row was picked) / T is a lottery over the rows under which agent i is selected with probability
 * d_cover[i] / T exactly, so the least of these over the agents some row holds is a LOWER bound on the optimum
 * z* (and on LEXIMIN's minimum probability: the drawn panels are some of the feasible ones); every weight
 * vector w met is a dual point, so z* <= the best score / the sum of w, the UPPER bound.  Stream-ordered; the
 * length is read on the device; nothing waits, nothing is allocated.
 *
 * Table, n, score, "best" (float64 values compared with >, ties to the lowest row) and the lane-strided sum
 * are the pricing entry points' above.  State, all caller-owned, read and written, so a second call continues
 * the first: d_weights float64[n]; d_scores float64[cap]; d_cover uint32[n]; d_row_count uint32[cap];
 * d_state uint64[4] = (bits of `upper`, rounds done, row of the last fresh best, bits of the last fresh ratio
 * u); d_picks uint32[rounds] or NULL.
 *
 * Start (CSA_MAXIMIN_START in flags): w[i] = 1.0 where some valid row holds agent i, else +0.0 (the
 * first-holder pass); cover, row_count, rounds done = 0; a fresh score pass over w writes the scores; U = the
 * best score, s = the lane-strided sum of w, upper = U / s (IEEE division); the state's row and u are that
 * pass's.  An empty table starts as (+inf, 0, CSA_PRICE_NONE, +inf) with all weights +0.0.
 *
 * Round r of a call (0-based) is FRESH when (r + 1) % resync == 0 or r == rounds - 1, so every call ends on
 * fresh scores and normalised weights.
 *   1. p = the first row holding the maximum of d_scores.
 *   2. d_picks[r] = p; d_row_count[p] += 1; d_cover[i] += 1 for the members of row p; rounds done += 1.
 *   3. For the members of row p: v = w[i] * shrink (one rounded multiply), delta[i] = w[i] - v (one rounded
 *      subtract, never an fma), w[i] = v.  For everyone else delta[i] = +0.0.
 *   4. Not fresh: for every valid row d, t = the sum of delta[i] over the set bits i of row_d & row_p in
 *      ascending i from +0.0, one rounded add each; d_scores[d] = d_scores[d] - t.
 *   5. Fresh: s = the lane-strided sum of w; f = (double)n / s; w[i] = w[i] * f for all i; a fresh score pass
 *      writes the scores; U = its best; s2 = the lane-strided sum of the new w; u = U / s2; upper = u if
 *      u < upper; u and the best row are recorded in the state.
 * An empty table writes 0xFFFFFFFF picks and changes nothing else.  rounds == 0 with CSA_MAXIMIN_START only
 * initialises; without it nothing is launched.  Launches: two per round, three on a fresh round, plain
 * launches on the caller's stream with no host wait between them; a call without CSA_MAXIMIN_START first
 * rebuilds its per-tile bests from d_scores, so the scratch need not survive between calls.
 * d_scratch: csa_rows_maximin_scratch_bytes(cap, W) bytes, 8-byte aligned (the per-tile bests, delta, the
 * first holders, two words).
 *
 * CSA_E_UNSUPPORTED for cap >= 2^32 - 1 or a W beyond the LDS.  CSA_E_INVALID, before any device call, for
 * what the pricing entry points refuse of the table and n, shrink outside [0.5, 1), resync outside [1, 64] (so
 * the weights between fresh rounds cannot underflow), unknown flags, a NULL d_weights / d_cover / d_state, a
 * NULL d_scores / d_row_count with cap > 0, state buffers that overlap each other, the table, the length or
 * the scratch, or a scratch that is NULL, short or misaligned. */
#define CSA_MAXIMIN_START 0x1u
uint64_t csa_rows_maximin_scratch_bytes(uint64_t cap, int32_t W);
int csa_rows_maximin_async(const uint64_t *d_rows, const uint64_t *d_len, uint64_t cap, int32_t W, int32_t n,
                           uint32_t rounds, double shrink, uint32_t resync, uint32_t flags, double *d_weights,
                           double *d_scores, uint32_t *d_cover, uint32_t *d_row_count, uint64_t *d_state,
                           uint32_t *d_picks /* or NULL */, void *d_scratch, uint64_t scratch_bytes, void *stream);

/* The per-agent marginals of a weighted table: pi = M^T p, agent i's selection probability under the lottery
 * that draws row d with probability d_prob[d].  Table, length and n as for csa_rows_price_async; a row past
 * min(*d_len, cap) is never loaded and its d_prob entry never read.
 * Summation-order contract (float64, no multiply, nothing to contract): the valid rows are cut into tiles of
 * csa_rows_nash_tile() = 1024 consecutive rows.  For tile b and agent i, part[b][i] = the sum from +0.0, in
 * ASCENDING row order, of d_prob[d] over the tile's valid rows that hold i: one rounded add per holder, a row
 * that does not hold i adds nothing.  d_marginals[i] = the sum from +0.0 over ascending b of part[b][i], for
 * i < n.  *d_psum = the same two-level sum over all valid rows.  A host loop gives the same bits
 * (stats.rows_marginals_host).  An empty table writes +0.0 everywhere.
 * d_scratch: csa_rows_marginals_scratch_bytes(cap, W) bytes, 8-byte aligned (the per-tile sums).  Two plain
 * launches on the caller's stream, no host wait, no allocation.
 * CSA_E_UNSUPPORTED for cap >= 2^32 - 1 or a W beyond the LDS of the pricing pass.  CSA_E_INVALID, before any
 * device call, for what the pricing entry points refuse of the table and n, a NULL d_marginals or d_psum, a NULL
 * d_prob with cap > 0, outputs that overlap each other, the inputs or the scratch, or a scratch that is NULL,
 * short or misaligned when cap > 0. */
uint32_t csa_rows_nash_tile(void);
uint64_t csa_rows_marginals_scratch_bytes(uint64_t cap, int32_t W);
int csa_rows_marginals_async(const uint64_t *d_rows, const uint64_t *d_len, uint64_t cap, int32_t W, int32_t n,
                             const double *d_prob, double *d_marginals, double *d_psum, void *d_scratch,
                             uint64_t scratch_bytes, void *stream);

/* The Nash-welfare lottery over a sorted table of drawn panels: row probabilities p that maximise the product
 * (the geometric mean) of the selection probabilities pi_i = the sum of p_d over the rows holding i, over the
 * m agents some valid row holds.  Cover's multiplicative iteration: G_d = the sum of 1 / pi_i over the members
 * of row d, p_d <- p_d * (G_d / m).  It keeps the sum of p at 1 in real arithmetic, raises the objective
 * monotonically from a start with full support, and its fixed point is the optimum.  With s = the sum of p,
 * ratio = (max_d G_d / m) * s bounds optimum / GM(pi / s) from above (Jensen), so after every round
 * GM(pi / s) <= optimum <= GM(pi / s) * ratio, and ratio -> 1.
 * State, all on the device, so that a call without CSA_NASH_START continues the previous one: d_prob
 * (float64[cap], p), d_scores (float64[cap], G), d_marginals (float64[n], pi) and d_state (uint64[4] = bits of
 * ratio, rounds done, the first row holding max G, bits of s) all belong to the same p after every round.
 * Contract, every step float64 and rounded once (no fused multiply-add anywhere); D = min(*d_len, cap):
 *   start (CSA_NASH_START): p[d] = (double)d_mult[d] / (double)total for d < D -- the run's own lottery when
 *      total is its number of draws --, or 1.0 / (double)D with a NULL d_mult.  Then the pass below; rounds
 *      done = 0.  Buffers need not be initialised.
 *   pass: pi and s by csa_rows_marginals_async's contract over p; inv[i] = 1.0 / pi[i] where some valid row
 *      holds i (m = how many do), else +0.0; G = csa_rows_price_async's scores under the weights inv (ascending
 *      agent index from +0.0); the best row = the first holding the greatest G; ratio = (G_best / (double)m) * s,
 *      the quotient rounded before the product.
 *   round: p[d] = p[d] * (G[d] / (double)m) for d < D, the quotient rounded before the product; the pass; rounds
 *      done += 1.
 * m > 0 is assumed of a table that has valid rows: a drawn panel has k >= 1 members.  Valid rows that are all
 * zero words give m = 0, and the quotients by m then put inf or NaN into p and the state; nothing refuses it, as
 * the table is on the device.
 * Nothing past D is read, scored or written in d_prob and d_scores.  An empty table: the start writes pi =
 * +0.0 and the state (+inf, 0, CSA_PRICE_NONE, +0.0); rounds change nothing.  rounds == 0 with CSA_NASH_START
 * only starts; without it nothing is launched.  Plain launches on the caller's stream (five a round), no
 * host wait, no allocation; every call rebuilds the first holders, so the scratch need not survive between
 * calls.  d_scratch: csa_rows_nash_scratch_bytes(cap, W) bytes, 8-byte aligned.
 *
 * CSA_E_UNSUPPORTED for cap >= 2^32 - 1 or a W beyond the LDS.  CSA_E_INVALID, before any device call, for
 * what the pricing entry points refuse of the table and n, unknown flags, a NULL d_marginals / d_state, a NULL
 * d_prob / d_scores with cap > 0, total == 0 with a non-NULL d_mult under CSA_NASH_START, state buffers that
 * overlap each other, the table, the multiplicities, the length or the scratch, or a scratch that is NULL,
 * short or misaligned. */
#define CSA_NASH_START 0x1u
uint64_t csa_rows_nash_scratch_bytes(uint64_t cap, int32_t W);
int csa_rows_nash_async(const uint64_t *d_rows, const uint64_t *d_len, uint64_t cap, int32_t W, int32_t n,
                        uint32_t rounds, uint32_t flags, const uint32_t *d_mult /* or NULL: uniform */,
                        uint64_t total, double *d_prob /* [cap] */, double *d_scores /* [cap] */,
                        double *d_marginals /* [n] */, uint64_t *d_state /* [4] */, void *d_scratch,
                        uint64_t scratch_bytes, void *stream);

/* Multi-GPU pair exchange: pack the upper triangle incl. the diagonal of the
 * n*n int64 pair counts row-major into n(n+1)/2 int32 (every count must be
 * < 2^31), and unpack it back (overwriting the upper triangle). */
int csa_pairs_pack_async(const int64_t *d_pairs, int32_t n, int32_t *d_packed, void *stream);
int csa_pairs_unpack_async(const int32_t *d_packed, int32_t n, int64_t *d_pairs, void *stream);

/* PairHistogram materialisation (replaces the host-side division and triangle walk of
 * analysis.py:86-98): the strict upper triangle (i < j, row-major -- the reference's key order,
 * analysis.py:70) of the n*n int64 pair counts, packed into n(n-1)/2 entries of d_out: float64
 * count / divisor (IEEE, correctly rounded: Python's int / int) for divisor > 0, int64 counts for
 * divisor == 0.  Stream-ordered. */
int csa_pairs_upper_async(const int64_t *d_pairs, int32_t n, double divisor, void *d_out, void *stream);

/* Per-person counts (agent_appearance_counter, analysis.py:179, 187) = the diagonal of the n*n int64
 * pair counts (every panel contributes x_i * x_i = x_i): d_counts[i] = d_pairs[i*n + i] (stored). */
int csa_pairs_diag_async(const int64_t *d_pairs, int32_t n, int64_t *d_counts, void *stream);

/* Portfolio probabilities: the work leximin_probabilities / xmin_probabilities do after the solver
 * returns (portfolio, probabilities) -- PairHistogram.add_portfolio_of_panels_to_histogram
 * (analysis.py:90-95) and the selection_probs loop (analysis.py:204-207, 222-225).  d_xt: the XT
 * planes of the portfolio's n_panels packed panels exactly as csa_transpose_count_async writes them;
 * d_weights: n_panels float64 probabilities in portfolio order.  Outputs (either may be NULL, not
 * both): d_upper, the strict upper triangle packed in the reference's key order (pair (i, j), i < j,
 * at i(n-1) - i(i-1)/2 + j-i-1; n(n-1)/2 float64), and d_alloc, the n per-person values (the
 * diagonal).
 * Summation-order contract: every output value starts from +0.0 -- with CSA_PORTFOLIO_ACCUMULATE
 * from the value stored in the output -- and receives d_weights[p] for each panel p that holds both
 * agents (the agent, for d_alloc), in ASCENDING p, one IEEE float64 addition each, as the reference's
 * `+=` per panel does: no reassociation, no tree reduction, no atomics, so the results are the
 * reference's floats bit for bit (float64 addition does not associate; a matrix product or a
 * reversed sum differs in the last bits).
 * Stream-ordered, no host wait.  n_panels == 0 leaves the outputs as they are with
 * CSA_PORTFOLIO_ACCUMULATE and zero-fills them without.  CSA_E_INVALID, before any device call, for
 * n < 0, a NULL d_xt or d_weights with n_panels > 0, both outputs NULL, or unknown flag bits. */
#define CSA_PORTFOLIO_ACCUMULATE 1u
int csa_portfolio_pairs_async(const uint64_t *d_xt, uint64_t n_panels, int32_t n, const double *d_weights,
                              double *d_upper /* n(n-1)/2 or NULL */, double *d_alloc /* n or NULL */,
                              uint32_t flags, void *stream);

/* Per-panel group composition: how many members of each agent group every panel holds, as one
 * histogram per group (quota features: how often a feature sits on its minimum or maximum;
 * two-feature intersections as in plot_intersectional_representation, analysis.py:459-530, which
 * can only take their mean from the marginals; households; any agent set).
 * hist[g*bins + c] += number of panels p in [0, n_panels) with popcount(panel_p & mask_g) == c.
 * d_panels: n_panels*W (csa_draw_async layout); d_masks: n_groups*W, agent p = bit p & 63 of word
 * p >> 6, padding bits zero; d_hist: n_groups*bins int64, ACCUMULATED (the caller zeroes it; chunks,
 * calls and ranks add).  A panel whose count >= bins writes nothing for that group and sets
 * CSA_E_INVALID (with the panel's index in this call) in d_status -- never a store outside d_hist;
 * every other (panel, group) is still counted.
 * Range: 1 <= W <= 8192 (one mask must fit 64 KB of LDS: CSA_E_UNSUPPORTED above, before any
 * launch), every bins >= 1 (the per-workgroup LDS table holds up to 160 KB - masks, i.e. about 380 bins
 * at W = 128; beyond that every count goes to d_hist directly, slower, same table), every
 * n_groups >= 0, n_panels <= 2^46.  n_panels == 0 or n_groups == 0 is a no-op.  Stream-ordered, no
 * host wait.  CSA_E_INVALID, before any device call, for W <= 0, n_groups < 0, bins < 1 or a NULL
 * pointer with work to do (d_status is required). */
int csa_group_hist_async(const uint64_t *d_panels, uint64_t n_panels, int32_t W, const uint64_t *d_masks,
                         int32_t n_groups, int32_t bins, int64_t *d_hist, uint32_t *d_status, void *stream);

/* Weighted group composition of a portfolio (LEXIMIN / XMIN): csa_group_hist_async's table with each
 * panel counted by its float64 weight, what LEGACY-versus-LEXIMIN comparisons at the panel level need
 * (how often a quota sits on its minimum, how often an intersection is absent); the marginals cannot
 * give it.  d_panels, d_masks, W, n_groups, bins as for csa_group_hist_async; d_weights: n_panels
 * float64 in portfolio order; d_hist: n_groups*bins float64.
 * Summation-order contract: hist[g*bins + c] starts from +0.0 -- with CSA_GROUP_WHIST_ACCUMULATE from
 * the stored value -- and receives d_weights[p] for every panel p with
 * popcount(panel_p & mask_g) == c, in ASCENDING p, one IEEE float64 addition each: no reassociation, no
 * tree reduction, no atomics on the values, no multiply.  A host loop over the panels gives the same
 * bits (stats.group_whist_host).  Without the flag every one of the n_groups*bins entries is written
 * (+0.0 where no panel lands); with it, entries no panel reaches keep their stored bits (a -0.0 stays
 * -0.0).  A panel whose count >= bins adds nothing for that group and sets CSA_E_INVALID (with the
 * panel's index) in d_status -- never a store outside d_hist; every other entry is still exact.
 * Scratch: the call runs two kernels, a parallel count pass (u32 counts[n_panels][n_groups]) and the
 * ordered sums over them; the counts go to a device buffer the caller lends beforehand with
 * csa_group_whist_scratch(d_scratch, bytes), bytes >= csa_group_whist_scratch_bytes(n_panels,
 * n_groups).  The loan is per calling thread and lasts until the next csa_group_whist_scratch call
 * (NULL, 0 ends it); the buffer must stay valid until the enqueued work has run, and calls that share
 * one buffer must be ordered on one stream.  Nothing is allocated by the enqueue.
 * Range: 1 <= W <= 8192 (CSA_E_UNSUPPORTED above, before any launch), every bins >= 1 (the rows sit in
 * LDS: 64 groups per workgroup to 302 bins, fewer beyond, one to 19 454; past that the row is d_hist
 * itself, same bits, slower),
 * n_panels < 2^40.  Stream-ordered, no host wait.  CSA_E_INVALID, before any device call, for W < 1,
 * bins < 1, n_groups < 0, unknown flag bits, a NULL pointer that is needed, or a scratch loan smaller
 * than csa_group_whist_scratch_bytes.  n_groups == 0 is a no-op; n_panels == 0 is a no-op with the
 * flag and sets the table to +0.0 without (only d_hist is needed then). */
#define CSA_GROUP_WHIST_ACCUMULATE 0x1u
uint64_t csa_group_whist_scratch_bytes(uint64_t n_panels, int32_t n_groups);
int csa_group_whist_scratch(void *d_scratch, uint64_t bytes);
int csa_group_whist_async(const uint64_t *d_panels, uint64_t n_panels, int32_t W, const double *d_weights,
                          const uint64_t *d_masks, int32_t n_groups, int32_t bins, double *d_hist,
                          uint32_t flags, uint32_t *d_status, void *stream);

/* Decode a device status block (host copy of the 4 words) into a CSA_* code
 * and set csa_last_error() accordingly. */
int csa_status_decode(const uint32_t *h_status);

#ifdef __cplusplus
}
#endif
#endif /* CSA_LEGACY_H */
