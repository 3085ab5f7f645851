/* dca_debug.h — test, tuning and profiling hooks of libdca_hip.so, kept apart from the product ABI (include/dca.h).
 *
 * Nothing here is needed to run a search, an update or a network forward: these entry points exist for tests/ (race screens
 * against a plain schedule, forced fallbacks, tiny tiers), for bench.py's device-side launch profile and for the measurement
 * tools under tools/ — and knob 5 of dca_debug_tune, which processes sharing one GPU set.  Same conventions as dca.h (plain C, int return codes, the error text of the last failure through dca.h).  Exported by the same library. */
#ifndef DCA_DEBUG_H
#define DCA_DEBUG_H

#include "dca.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- engine ------------------------------------------------------------------------------------------------------ */
/* Host-only (no device needed): the chunk dca_engine_run_builtin would replay as ONE hipGraph for a run of `remaining`
 * iterations starting at iteration `host_iter` of a search — its length n (<= 64: up to the next rebase-period boundary, then
 * whole periods) and which of its iterations are rebase iterations (bit i of rebase_mask).  For tests of the cutting rule. */
int dca_engine_plan_chunk(int64_t host_iter, int remaining, int* n, uint64_t* rebase_mask);

/* Host-only (no device needed): does the engine's expansion skip the CLOSED probe for the child by move `action` of a node with
 * path cost g_parent that was made by move move_parent (0xFF: the root)?  1 = yes (a known duplicate: the undo child from
 * g_parent >= 2, a sliding puzzle's ineligible move from g_parent >= 1), 0 = no.  The rule the kernel evaluates, for tests.
 * env / dim as the engine instantiates them (cube3 / 0, lightsout / 7, sliding puzzles / 3..7); blank = position of the
 * puzzle's blank in the parent (ignored for the other environments).  DCA_E_BADARG for anything out of range.            */
int dca_engine_known_duplicate(int env, int dim, int64_t g_parent, int move_parent, int action, int blank);

/* Device-side profile of `iters` iterations of run_builtin (use_graph as there): every workgroup stamps the device wall
 * clock at entry and exit, per launch the host takes max(end) - min(start) as the launch's busy span and the distance to
 * the previous launch's end as the gap in front of it — measured INSIDE the replayed hipGraph, which HIP events between
 * eager launches cannot do.  span_ms / gap_ms: host float[DCA_PROF_SLOTS], summed milliseconds over the iterations
 * (gap_ms may be NULL).  Slots: 0 refill_hist 1 refill_scan 2 refill_move 3 sel_hist (= the FRONT rebase pass; 0-3 only in
 * rebase iterations: every 8th, and the first twelve after a reset) 4 sel_scan 5 sel_collect 6 rank 7 expand (with the CLOSED
 * probe) 8 unused (stays empty: the slot numbers do not move) 9 decide 10 pack (dedup-first stepping only) 11 commit; 12 / 13 = the two halves of the rank launch (small-bin pass, large-bin
 * workgroups), 14-17 = phases of the large-bin path (load + range, count + prefix, scatter, order) as envelopes over the
 * workgroups — for tuning.  Synchronises every iteration.                                                            */
#define DCA_PROF_SLOTS 18
int dca_engine_profile_builtin(dca_engine* e, int heur_id, int iters, int use_graph, float* span_ms /*host [DCA_PROF_SLOTS]*/,
                               float* gap_ms /*host [DCA_PROF_SLOTS] or NULL*/, void* stream);

/* test / tuning hook: FRONT-tier hysteresis in entries (defaults 32*B / 96*B); results never depend on it */
int dca_engine_set_tiers(dca_engine* e, int64_t front_keep, int64_t front_max);

/* internals of the last iteration for diagnostics (host double[16]; layout in dca_engine.hip); synchronises */
int dca_engine_debug(dca_engine* e, double* out /*host [16]*/, void* stream);
/* Sets one of the engine's three hooks process-wide (value 0 = the shipped behaviour):
 *   2: BACK is squeezed without a refill once it holds more than max_nodes * value / 1024 physical entries (tests: the
 *      compaction-only pass under tiny tiers);
 *   5: value != 0 turns the grid-wide refinement of giant tie bins off for every engine created afterwards (host side, no
 *      device needed).  search_methods/sharding.py sets it when several processes share one GPU: that path needs every
 *      workgroup of its launch resident, which such processes cannot promise each other;
 *   10: value != 0 makes the first grid barrier of every giant iteration give up at once (tests: the consensus fallback that
 *      dca_engine_info [4] reports).
 * Any other knob is refused with DCA_E_BADARG (the error text names it) before any HIP call.                             */
int dca_debug_tune(int knob, int value);

/* ---- IDA* --------------------------------------------------------------------------------------------------------- */
/* Host-only (no device needed): the search of dca_idastar_npuzzle — env DCA_ENV_NPUZZLE, dim 3..5; kinds ignored, may be NULL —
 * or of dca_idastar_cube3 — env DCA_ENV_CUBE3; dim ignored — run sequentially on the CPU from tables in HOST memory, through the
 * same move, index-update, pruning and work-item code the kernel compiles.  Same refusals, same outputs; the completed
 * iterations' thresholds and node counts equal the device's.  For tests on a machine without a GPU. */
int dca_idastar_host(int env, int dim, const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* ids, const int* ks,
                     const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int64_t max_nodes, int* status, int* length,
                     uint8_t* moves, int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold,
                     int thresholds_cap, int64_t* total_nodes);
/* Host-only: the search of dca_idastar_npuzzle_reflected on the CPU from HOST tables, as dca_idastar_host is that of
 * dca_idastar_npuzzle.  Same refusals (num_patterns in 1..4), same outputs. */
int dca_idastar_host_reflected(int dim, const uint8_t* root, int num_patterns, const uint8_t* tiles, const int* ks,
                               const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int64_t max_nodes, int* status,
                               int* length, uint8_t* moves, int moves_cap, int* num_thresholds, int* thresholds,
                               int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes);
/* Host-only: the batch of dca_idastar_npuzzle_batch on the CPU from HOST tables: the same driver and rounds, a round's roots run
 * one after the other on the sequential search of dca_idastar_host (reflect != 0: of dca_idastar_host_reflected).  Same
 * refusals, same outputs. */
int dca_idastar_host_batch(int dim, const uint8_t* roots /*host [n_roots, N]*/, int n_roots, int num_patterns, const uint8_t* tiles,
                           const int* ks, const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int reflect,
                           int64_t max_nodes, int* status, int* length, uint8_t* moves, int moves_cap, int* num_thresholds,
                           int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes);
/* Host-only: what dca_pdb_eval computes where reflect == 0, what dca_pdb_eval_reflected computes otherwise, in a plain loop on
 * the CPU, through the row load and the row value the kernels compile.  states, tables and out are HOST memory; the refusals are those of dca_pdb_eval.
 * So that the any-bytes rule and the reflected index have a test on a machine without a GPU. */
int dca_pdb_eval_host(int dim, const uint8_t* states /*host [n, ld]*/, int64_t n, int64_t ld, int num_patterns,
                      const uint8_t* tiles /*host*/, const int* ks /*host [num_patterns]*/,
                      const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int reflect, float* out /*host [n]*/);
/* Host-only: the search of dca_idastar_cube3_sym on the CPU from HOST tables, through the code the kernel compiles.  Same
 * refusals, same outputs; the thresholds and the completed iterations' node counts equal the device's. */
int dca_idastar_host_sym(const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                         const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int max_images, int64_t max_nodes,
                         int* status, int* length, uint8_t* moves, int moves_cap, int* num_thresholds, int* thresholds,
                         int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes);
/* Host-only: what dca_cube3_pdb_eval_sym computes, in a plain loop on the CPU through the row load and the row value the kernel
 * compiles.  states, tables and out are HOST memory; the refusals are those of dca_cube3_pdb_eval_sym. */
int dca_cube3_pdb_eval_sym_host(const uint8_t* states /*host [n, ld]*/, int64_t n, int64_t ld, int row_kind, int num_patterns,
                                const int* kinds, const uint8_t* cubies, const int* ks,
                                const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int max_images,
                                float* out /*host [n]*/);
/* Host-only: the search of dca_idastar_cube3_dual on the CPU from HOST tables, through the code the kernel compiles.  Same
 * refusals, same outputs; the thresholds and the completed iterations' node counts equal the device's. */
int dca_idastar_host_dual(const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                          const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int max_images, int64_t max_nodes,
                          int* status, int* length, uint8_t* moves, int moves_cap, int* num_thresholds, int* thresholds,
                          int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes);
/* Host-only: the bounded batch of dca_idastar_cube3_batch on the CPU from HOST tables: the same driver, rounds and bounds, a
 * round's roots run one after the other on the sequential search of dca_idastar_host, dca_idastar_host_sym or
 * dca_idastar_host_dual.  Same arguments but the stream, same refusals, same outputs. */
int dca_idastar_host_cube3_batch(const uint8_t* roots /*host [n_roots, 54]*/, int n_roots, int num_patterns, const int* kinds,
                                 const uint8_t* cubies, const int* ks, const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/,
                                 int max_images /*0: plain*/, int dual, const int* max_length /*host [n_roots] or NULL*/,
                                 int64_t max_nodes, int* status, int* length, uint8_t* moves, int moves_cap, int* num_thresholds,
                                 int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes);
/* Host-only: what dca_cube3_pdb_eval_dual computes, in a plain loop on the CPU through the row load and the row value the kernel
 * compiles.  states, tables and out are HOST memory; the refusals are those of dca_cube3_pdb_eval_dual. */
int dca_cube3_pdb_eval_dual_host(const uint8_t* states /*host [n, ld]*/, int64_t n, int64_t ld, int row_kind, int num_patterns,
                                 const int* kinds, const uint8_t* cubies, const int* ks,
                                 const uint8_t* const* tables /*host [num_patterns] of HOST pointers*/, int max_images,
                                 float* out /*host [n]*/);
/* Host-only: the inversion rule of dca.h "Dual look-ups" in its replacing form on one row of 54 bytes (any bytes): words[0] =
 * the corner word, words[1] = the edge word of the inverse, 5 bits a cubie. */
int dca_cube3_inverse_locs(const uint8_t* row /*host [54]*/, int row_kind, uint64_t* words /*host [2]*/);
/* Host-only: the derived symmetries (dca.h "Symmetric look-ups"), in their documented order: sticker_perms [48][54], sigma as
 * position -> position; move_maps [48][12], pi.  DCA_E_STATE where the derivation failed its checks. */
int dca_cube3_sym_tables(uint8_t* sticker_perms /*host [48*54]*/, uint8_t* move_maps /*host [48*12]*/);
/* Host-only: the images of one pattern as the look-up list holds them, the first min(max_images, distinct) of them:
 * *num_images; per image i the symmetry that stands for it, syms[i]; its source cubies, sources[i*8 + j] for j < k; and their
 * location maps, maps[(i*8 + j)*24 + l].  syms, sources and maps may each be NULL; room for 48 images.  The refusals of a
 * pattern (dca_cube3_pdb_bytes, cubies) and of max_images. */
int dca_cube3_sym_images(int kind, const uint8_t* cubies /*host [k]*/, int k, int max_images, int* num_images,
                         uint8_t* syms /*host [48] or NULL*/, uint8_t* sources /*host [48*8] or NULL*/,
                         uint8_t* maps /*host [48*8*24] or NULL*/);
/* test hook, process-wide: every iteration of the searches above splits its work into items of `depth` prefix moves (a
 * family's own limit where depth is above it: 15 for the puzzles, 6 for cube3); -1 (the default) = chosen from the previous
 * iteration's node count.  Results never depend on it.  DCA_E_BADARG outside -1..15.
 * NOT thread-safe: one plain global that the production entry points read at every iteration.  Never call it while a search
 * runs in another thread, and put -1 back before anything but a test searches. */
int dca_idastar_set_prefix(int depth);

/* ---- environment kernels ------------------------------------------------------------------------------------------- */
/* Store-only yardstick of the gather kernel's roofline (bench.py times it in the same process, right after the kernel itself):
 * fills buf[0, bytes) with plain 16-byte stores, one contiguous region of bytes_per_block per workgroup (1 MiB: the pattern
 * tools/hbm_write_ceiling.hip found best on an MI355X).  buf 16-byte aligned; bytes and bytes_per_block multiples of 16. */
int dca_debug_write_ceiling(void* buf, int64_t bytes, int64_t bytes_per_block, void* stream);

/* ---- dense-layer kernels: schedule selectors (the race screens compare the default schedule with a plain one) --------- */
/* dca_f16x3_gemm */
/* test hook: 3 (default) = 256 x 256 tiles filled by LDS-DMA on the ping-pong / half-tile schedule (two wave groups one barrier
 * apart, the DMA queue never drained); 2 = the same tile with two whole-K-step stages and one drain + barrier per K-step
 * (bit-identical to 3: same products in the same order — what the race screens in tests/ compare against).  ldo % 4 == 0,
 * out_h / out_l 8-byte and x_out / skip 16-byte aligned. */
int dca_f16x3_gemm_variant(int variant);

/* dca_gemm16 */
/* test hook: 3 (default) = the 8-phase schedule (two wave groups one barrier apart, half-tile staging, the DMA queue never
 * drained) with the MFMA operand roles swapped and a lean tail compiled per layer form — relu(a . w^T + bias (+ skip)) on whole
 * 256 x 256 tiles with 16-byte aligned rows; other forms and the ragged strips of a layer run on 2 = the same schedule with the
 * general tail; 1 = two whole K-step stages with one drain + barrier per K-step (the plain reference of the race screens).
 * Bit-identical results (same products, same accumulation order). */
int dca_gemm16_variant(int variant);

#ifdef __cplusplus
}
#endif
#endif /* DCA_DEBUG_H */
