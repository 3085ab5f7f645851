/*
 * dca.h — C ABI of libdca_hip.so, the MI355X (gfx950) batched weighted-A* (BWAS)
 * node-expansion engine for DeepCubeA-style search.
 *
 * This header is the drop-in boundary.  Every entry point names the
 * reference interface it replaces (paths relative to forestagostinelli/DeepCubeA):
 *
 *   environments/environment_abstract.py:23-163   Environment API (Python, in-process)
 *   environments/cube3.py:48-171                  Cube3.next_state/prev_state/expand/is_solved/state_to_nnet_input
 *   environments/n_puzzle.py:46-231               NPuzzle.*  (same set)
 *   utils/pytorch_models.py:49-52                 F.one_hot(x.long(), depth).float().view(-1, D*depth)
 *   cpp/environments.cpp:92-126,222-256           C++ twins (PuzzleN / Cube3 getNextState, isSolved)
 *   cpp/parallel_weighted_astar.cpp:138-346       the native BWAS loop (argv/stdout/socket boundary, replaced)
 *   search_methods/astar.py:50-90,232-340         Instance / AStar (python BWAS semantics)
 *
 * Conventions
 *   - plain C, no torch / STL types.  All `const uint8_t*` / `void*` buffers are
 *     caller-owned DEVICE memory unless the parameter comment says "host".
 *   - every call takes a hipStream_t (passed as void*) and is stream-ordered and
 *     asynchronous unless documented otherwise; the library never frees or
 *     reallocates caller memory.
 *   - return value: 0 = ok, >0 = hipError_t, <0 = library error (DCA_E_*);
 *     dca_last_error() returns a thread-local message for the last failure.  An
 *     argument check that fails returns DCA_E_BADARG before any device call, and the
 *     message is "bad argument: <entry point>: <the condition that failed>".
 *   - state rows are row-major uint8: cube3 [n,54] sticker ids 0..53; puzzles
 *     [n,dim*dim] tile ids 0..dim*dim-1 (0 = blank) — the reference's own numpy layout.
 */
#ifndef DCA_H_
#define DCA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Still 6 with puzzle8: no signature changed; only the accepted range of every puzzle `dim` argument grew from 4..7 to 3..7
 * (a refusal names the range: "unsupported puzzle dim %d (3..7)"), and the layer-1 geometry (9, 9) joined the instantiated ones. */
#define DCA_ABI_VERSION 6

/* library error codes (negative; positive values are hipError_t) */
#define DCA_E_BADARG (-1)
#define DCA_E_NOMEM (-2)
#define DCA_E_CAPACITY (-3) /* node pool / closed table / OPEN exhausted */
#define DCA_E_STATE (-4)    /* call sequence violated (e.g. commit before pop_expand) */
#define DCA_E_NOTFOUND (-5)

/* environments (utils/env_utils.py:6-28 registry names) */
#define DCA_ENV_CUBE3 0   /* "cube3": 54 stickers, 12 moves */
#define DCA_ENV_NPUZZLE 1 /* "puzzle8/15/24/35/48": dim 3..7, 4 moves U D L R */
#define DCA_ENV_LIGHTSOUT 2 /* "lightsout7": dim 7, 49 cells in {0,1}, 49 moves (press cell a: it and its 4-neighbours flip) */
#define DCA_ENV_CUBE4 3   /* the 4x4x4 cube of the reference's C++ core (cpp/environments.cpp:263-370): 96 stickers, 24 moves
                           * (12 outer-layer turns, then 12 inner-slice turns; move a^1 is the inverse of move a); solved =
                           * every face shows one colour (sticker / 16).  Environment kernels only: the reference's Python
                           * harness has no Cube4 (astar.py:473-486), so there is no network input / search driver for it. */

/* one-hot element types for the fused encoder (utils/pytorch_models.py:49-52 emits f32) */
#define DCA_DT_F32 0
#define DCA_DT_F16 1
#define DCA_DT_BF16 2
/* (3 is unused: dca_l1_onehot_gemm refuses it) */
#define DCA_DT_F16_PLANES 4 /* dca_l1_onehot_gemm only: dca_f16x3_gemm's operand — [m, n_pad] fp16 high halves, then [m, n_pad] low halves */
#define DCA_DT_E4M3 5 /* dca_l1_onehot_gemm only: OCP fp8 e4m3 bytes, saturating (dca_gemm8's operand; the caller folds the activation
                         scale into the layer's weights and bias) */
#define DCA_DT_F64 6  /* dca_head_gemv only: float64 rows (the fp64 mode's residual stream) */

/* BWAS semantics: which reference implementation is reproduced */
#define DCA_SEM_PY 0  /* search_methods/astar.py: f64 cost, FIFO ties, CLOSED starts empty */
#define DCA_SEM_CPP 1 /* cpp/parallel_weighted_astar.cpp: f32 cost, root in CLOSED, deferred stop.  PARITY UNPINNED beyond
                         * four recorded answers of the reference binary (the binary needs boost and
                         * cannot be rebuilt here): moves, path cost, iterations and nodes generated match them; |OPEN| /
                         * |CLOSED| may differ < 1 % where equal float32 costs tie (std::priority_queue's tie order is
                         * unspecified; this library breaks ties by push order).  DCA_SEM_PY is the exact one. */

/* built-in deterministic heuristics (test / engine-only benchmarking) */
#define DCA_HEUR_MOD97 0  /* f32( ((sum_i s_i*(7i+3)) mod 97) ) / 50f                        */
#define DCA_HEUR_KNUTH3 1 /* f32( ((sum_i s_i*(7i+3)) * 2654435761 mod 2^32) / 2^32 * 3 )    */
#define DCA_HEUR_HASHU01 2 /* f32( 10 + 5 * (hash64(s) >> 11) / 2^53 )                        */
#define DCA_HEUR_ZERO 3   /* 0 (uniform-cost search; nnet_utils.py:271-272 all_zeros server) */
#define DCA_HEUR_MANHATTAN 4 /* puzzles: sum over tiles of |row-row*|+|col-col*| (admissible, consistent); cube3: 0 */

int dca_abi_version(void);
const char* dca_last_error(void);

/* ---- move tables (host pointers, static storage) -------------------------------------- */
/* cube3 gather map: next[i] = cur[perm[a*54+i]]  (≡ cube3.py:183-256 / environments.h:75-105) */
const uint8_t* dca_cube3_perm_table(void);                 /* [12*54] */
/* puzzle blank-swap table [dim*dim*4] (≡ n_puzzle.py:174-214 / environments.cpp:4-46) */
int dca_npuzzle_swap_table(int dim, uint8_t* out /*host [dim*dim*4]*/);

/* ---- a1,a2: single-action move (Cube3._move_np cube3.py:163-171; prev = action^1) ------ */
int dca_cube3_next_state(const uint8_t* in /*[n,54]*/, int64_t n, int action, uint8_t* out /*[n,54]*/, void* stream);
int dca_cube3_prev_state(const uint8_t* in, int64_t n, int action, uint8_t* out, void* stream);
/* a7: NPuzzle._move_np (n_puzzle.py:216-231); blank index recomputed per state like n_puzzle.py:51-53 */
int dca_npuzzle_next_state(const uint8_t* in /*[n,dim*dim]*/, int64_t n, int dim, int action, uint8_t* out, void* stream);
int dca_npuzzle_prev_state(const uint8_t* in, int64_t n, int dim, int action, uint8_t* out, void* stream);

/* LightsOut._move_np (lights_out.py:155-166) / LightsOut::getNextState (environments.cpp:168-180): pressing cell `action`
 * flips it and its in-board 4-neighbours (move matrix lights_out.py:33-44 / environments.cpp:133-154).  Every move is
 * its own inverse: prev_state == next_state (lights_out.py:52-53).  dim 7 ("lightsout7", the only size the reference's
 * C++ core and train.sh use). */
int dca_lightsout_next_state(const uint8_t* in /*[n,dim*dim]*/, int64_t n, int dim, int action, uint8_t* out, void* stream);

/* ---- a3-a6,a9: fused expansion -----------------------------------------------------------
 * One launch: all children of every parent (Cube3.expand cube3.py:129-161), plus — each
 * optional, pass NULL to skip — the network input colour index (state_to_nnet_input
 * cube3.py:77-85: sticker//9), its one-hot encoding (pytorch_models.py:49-52; row = pos*6+colour),
 * is_solved (cube3.py:71-75) and the 64-bit state hash defined below.
 * Output order everywhere: child index = parent*num_moves + move.                           */
int dca_cube3_expand_fused(const uint8_t* parents /*[n,54]*/, int64_t n,
                           uint8_t* children /*[n,12,54] or NULL*/,
                           uint8_t* color_idx /*[n*12,54] or NULL*/,
                           void* onehot /*[n*12,324] of onehot_dtype or NULL*/, int onehot_dtype,
                           uint8_t* is_solved /*[n*12] or NULL*/,
                           uint64_t* hash /*[n*12] or NULL*/, void* stream);
/* puzzles: nnet input = the tiles themselves (n_puzzle.py:84-89); one-hot depth dim*dim */
int dca_npuzzle_expand_fused(const uint8_t* parents /*[n,D]*/, int64_t n, int dim,
                             uint8_t* children /*[n,4,D] or NULL*/,
                             void* onehot /*[n*4,D*D] or NULL*/, int onehot_dtype,
                             uint8_t* is_solved /*[n*4] or NULL*/,
                             uint64_t* hash /*[n*4] or NULL*/, void* stream);

/* lightsout: nnet input = the cells themselves (lights_out.py:70-75); one-hot depth 6 (get_nnet_model, lights_out.py:80) */
int dca_lightsout_expand_fused(const uint8_t* parents /*[n,D]*/, int64_t n, int dim,
                               uint8_t* children /*[n,D,D] or NULL*/,
                               void* onehot /*[n*D,D*6] or NULL*/, int onehot_dtype,
                               uint8_t* is_solved /*[n*D] or NULL*/,
                               uint64_t* hash /*[n*D] or NULL*/, void* stream);

/* cube4 — the remaining environment of the reference's C++ core (cpp/environments.cpp:263-370, tables environments.h:125-145):
 * 96 stickers (face * 16 + row * 4 + col), 24 moves; getNextState = a permutation gather (perm_table: next[i] =
 * cur[perm[a][i]], [24][96]), prev_state(a) = next_state(a ^ 1), isSolved = every face shows one colour (sticker / 16).
 * The reference's Python harness cannot drive Cube4 (astar.py:473-486 has no state_dim for it): no network input, no one-hot,
 * no engine instantiation here either — the environment kernels (the DCA_ENV_CUBE4 instantiation of the same tile code). */
const uint8_t* dca_cube4_perm_table(void);
int dca_cube4_next_state(const uint8_t* states /*[n,96]*/, int64_t n, int action, uint8_t* out, void* stream);
int dca_cube4_prev_state(const uint8_t* states, int64_t n, int action, uint8_t* out, void* stream);
int dca_cube4_expand_fused(const uint8_t* parents /*[n,96]*/, int64_t n, uint8_t* children /*[n,24,96] or NULL*/,
                           uint8_t* is_solved /*[n*24] or NULL*/, uint64_t* hash /*[n*24] or NULL*/, void* stream);

/* ---- stand-alone pieces of the same path (used by the Environment mirror) --------------- */
int dca_is_solved(int env, int dim, const uint8_t* states, int64_t n, uint8_t* out /*[n]*/, void* stream);
int dca_hash64(const uint8_t* states, int64_t n, int state_dim, uint64_t* out /*[n]*/, void* stream);
/* cube3: color_idx[n,54] = states//9 ; puzzles: copy */
int dca_nnet_input(int env, int dim, const uint8_t* states, int64_t n, uint8_t* out, void* stream);
/* generic one-hot of a [n,D] uint8 index array with depth `depth` -> [n, D*depth] */
int dca_onehot(const uint8_t* idx, int64_t n, int state_dim, int depth, void* out, int dtype, void* stream);
/* built-in deterministic heuristics on raw states -> f32 */
int dca_heuristic_builtin(int heur_id, const uint8_t* states, int64_t n, int state_dim, float* out, void* stream);

/* ---- (f)-1: approximate-value-iteration update step (ctg_approx/avi.py:129-159 do_update) -----------
 * generate_states (cube3.py:96-127 / n_puzzle.py:100-134): state i = goal after k_i ~ U{back_lo..back_hi}
 * uniformly random REVERSE moves; counter-based RNG keyed by (seed, index0 + i, step) so shards are
 * reproducible and independent.  out_num_back[n] / out_moves[n, moves_stride] (the forward move undone at
 * each step, -as taken-) are optional (NULL).                                                        */
int dca_generate_states(int env, int dim, int64_t n, int back_lo, int back_hi, uint64_t seed, int64_t index0,
                        uint8_t* out_states /*[n,D]*/, int32_t* out_num_back, int8_t* out_moves, int moves_stride,
                        void* stream);
/* search_utils.bellman (search_utils.py:16-32) after the children were expanded and evaluated:
 * ctg_backup[i] = solved_parent[i] ? 0 : min_a(1 + h[i*A+a]) (max(h,0) first when clip_zero),
 * argmin[i] = first a attaining it (gbfs.py:108 np.argmin).  Either output may be NULL.            */
int dca_bellman_backup(const float* h_children /*[n*A]*/, const uint8_t* solved_parent /*[n] or NULL*/, int64_t n,
                       int num_moves, int clip_zero, float* ctg_backup /*[n]*/, int32_t* argmin /*[n]*/, void* stream);

/* Heuristic cache of the update step (csrc/dca_hcache.hip; `--update_cache`, DCA_UPDATE_CACHE): updaters/updater.py:11-54 hands
 * all n x moves children of a batch to the target network although many are the same state.  This is a device-resident table
 * keyed by the uint8 network-input row so that every distinct row is evaluated once.  It is EXACT only for a batch-invariant
 * heuristic — a row's value has the same bits in any batch, row position or chunking: the fp32 parity network and the fp64
 * mode; a network that calibrates on the batch it sees (fp8) must not be cached.
 * The table is caller-owned device memory, 16-byte aligned, dca_hcache_bytes(row_bytes, slots) bytes (a pure function of its
 * arguments: 64 + slots * (24 + 8 * ceil(row_bytes / 8)); DCA_E_BADARG unless row_bytes is 1..64 and slots a power of two in
 * 2..2^30); all zero bytes = empty (dca_hcache_clear).  The rule:
 *   tag       a slot's tag is dca_hash64 of the row (the hash defined below, D = row_bytes); tag 0 means empty, so a row that
 *             hashes to 0 is never cached (EVAL_ONLY).
 *   probing   the start slot is hash & (slots - 1); linear probing, at most 32 probes; an empty slot is claimed by one 64-bit
 *             compare-and-swap of the tag.
 *   fill limit  no slot is claimed once slots / 2 are in use; after that the table only answers.  A claim takes its place in
 *             the count before the compare-and-swap and gives it back when it loses, so the count never passes slots / 2; a
 *             row may therefore be turned away early (EVAL_ONLY, still correct) while the stored keys plus the rows of the
 *             call in flight exceed slots / 2.
 *   equality is the bytes, not the hash: a row whose tag matches is compared byte for byte with the slot's stored row before
 *             it may share its value.
 * dca_hcache_lookup sets one status per row (rows [n, row_bytes], row stride ld >= row_bytes bytes, any byte alignment):
 *   DCA_HCACHE_HIT         h[i] is filled from the table;
 *   DCA_HCACHE_EVAL_STORE  the first row of a new key in this call: the caller evaluates it and writes h[i];
 *   DCA_HCACHE_DUP         the same bytes as an EVAL_STORE row of this call;
 *   DCA_HCACHE_EVAL_ONLY   the row cannot be cached; the caller evaluates it and nothing is stored: the probe limit or the fill
 *                          limit was reached, the tag matched but the bytes differ, or the key was claimed by an earlier call
 *                          that never stored a value.
 * slot[i] = the row's slot, -1 for EVAL_ONLY; h[i] is written for HIT rows only.  Which of several equal rows becomes the
 * EVAL_STORE one is left to the race; no output depends on it, because a value is a function of the row alone.
 * dca_hcache_finish (after the caller wrote h[i] of every EVAL_STORE and EVAL_ONLY row) first stores the EVAL_STORE values,
 * then fills the DUP rows; every slot index it reads back is range-checked.  One lookup / finish pair at a time per table.
 * No thread ever waits for another thread's write (what one must see of another is separated by a kernel boundary: lookup
 * and finish are two launches each), there are no spin loops, every loop has a fixed bound.  n == 0 launches nothing; n < 2^31.
 * DCA_E_BADARG before any device call: row_bytes outside 1..64, slots not a power of two, n < 0, ld < row_bytes, then a NULL
 * or misaligned table / output. */
#define DCA_HCACHE_HIT 0
#define DCA_HCACHE_EVAL_STORE 1
#define DCA_HCACHE_DUP 2
#define DCA_HCACHE_EVAL_ONLY 3
int64_t dca_hcache_bytes(int row_bytes, int64_t slots);
int dca_hcache_clear(void* table, int row_bytes, int64_t slots, void* stream);
int dca_hcache_lookup(void* table, int row_bytes, int64_t slots, const uint8_t* rows /*[n, ld]*/, int64_t n, int64_t ld,
                      float* h /*[n]*/, int32_t* slot /*[n]*/, uint8_t* status /*[n]*/, void* stream);
int dca_hcache_finish(void* table, int row_bytes, int64_t slots, int64_t n, const int32_t* slot /*[n]*/,
                      const uint8_t* status /*[n]*/, float* h /*[n]*/, void* stream);

/* Pattern databases for the sliding puzzles (csrc/dca_pdb.hip; `--model_dir pdb:<spec>`): additive disjoint pattern databases,
 * the exact admissible heuristic the paper measures its network against.  For a dim x dim board (dim 3..7, N = dim * dim) a
 * PATTERN is an ordered list of k distinct tiles from 1..N-1; its table is caller-owned device memory of dca_pdb_bytes(dim, k) =
 * N^(k+1) bytes (a pure function; DCA_E_BADARG unless dim is 3..7, k is 1..N-1 and the result is <= 2^34).
 *   index rule   index = blank_pos + N * (pos(tiles[0]) + N * (pos(tiles[1]) + ...)): the blank is the lowest digit, tiles[j] is
 *                digit j + 1.
 *   cost rule    table[index] = the smallest number of moves OF THE PATTERN'S TILES that takes the abstract state (the positions
 *                of these tiles and of the blank, every other tile invisible) to the goal — tile t at position t - 1, the blank
 *                at N - 1.  A blank move that swaps with a pattern tile costs 1, with an invisible tile 0.
 *   0xFF rule    an index with two digits equal is not a state and holds 0xFF.  A state the goal cannot be reached from holds
 *                0xFE; there are such states only where the pattern leaves at most one tile out (k >= N - 2: the visible tiles
 *                then fix the permutation's parity).  Every distance is far below 0xFE.
 * The blank stays in the index on purpose: the sum over DISJOINT patterns is then admissible (each move moves one tile, which
 * belongs to at most one pattern) and consistent (a move changes one pattern's abstract state along one of its edges, by at
 * most that edge's cost, and every other pattern's along a 0-cost edge of its own graph: |h(s) - h(s')| <= 1); the usual
 * minimum over blank positions is smaller and can be inconsistent.  One-tile patterns give exactly the Manhattan distance.
 * dca_pdb_build fills `table` by relaxation sweeps (one thread per entry pulls from its blank-move neighbours and writes only its
 * own byte; the fixed point has the same bits on every run) and SYNCHRONISES the stream once per sweep to read a "changed" word;
 * *sweeps (host, or NULL) = the sweeps it took, the last, unchanged one included.  tiles: host [k].
 * dca_pdb_eval: out[i] = sum over the set's patterns of table_p[index_p(row i)], an integer <= 24 * 255, exact in fp32.  states:
 * device rows [n, ld], ld >= N, any byte alignment; tiles: host, the patterns' tile lists one after another; ks: host
 * [num_patterns]; tables: HOST array of num_patterns device pointers.  The metadata travels as kernel arguments; stream-ordered,
 * nothing synchronises.
 *   partition    tiles in 1..N-1; no tile twice across the whole set; at most 24 patterns; a set that leaves tiles out is
 *                allowed (it is still admissible).
 *   any-bytes rule  the engine hands this call rows padded up to a multiple of 1024 whose padding is stale or all zero, so it is
 *                in bounds for ANY bytes: pos(t) of a row = the LAST position p < N with row[p] == t, 0 if there is none; bytes
 *                >= N match no tile.  Every digit is then < N and every index < N^(k+1) by construction.  The value of a row
 *                that is no permutation is whatever the tables hold there, 0xFF and 0xFE terms included, and is deterministic.
 * DCA_E_BADARG before any launch, the message naming the argument: dim outside 3..7; k outside 1..N-1 or a table over 2^34
 * bytes; a tile that is 0, >= N or named twice (build: within the pattern; eval: across the set); num_patterns outside 1..24; a
 * NULL tiles / ks / tables / table / out (states and out may be NULL when n == 0); ld < N; n < 0 or >= 2^31. */
int64_t dca_pdb_bytes(int dim, int k);
int dca_pdb_build(int dim, const uint8_t* tiles /*host [k]*/, int k, uint8_t* table /*device [N^(k+1)]*/, int* sweeps /*host or NULL*/,
                  void* stream);
int dca_pdb_eval(int dim, const uint8_t* states /*[n, ld]*/, int64_t n, int64_t ld, int num_patterns, const uint8_t* tiles /*host*/,
                 const int* ks /*host [num_patterns]*/, const uint8_t* const* tables /*host [num_patterns] of device pointers*/,
                 float* out /*[n]*/, void* stream);

/* Reflected look-up (Korf & Felner 2002): the goal — tile t at position t - 1, the blank at N - 1 — is its own mirror image in the
 * board's main diagonal, so mirroring a state keeps its distance, and the same tables read at the mirrored state give a second
 * admissible, consistent value at no table bytes.  For a dim x dim board, N = dim * dim:
 *   refl(p) = (p mod dim) * dim + p div dim      on positions
 *   phi(0) = 0, phi(t) = refl(t - 1) + 1         on tiles; both are involutions.
 * The mirror image of a state holds phi(t) at refl(pos(t)), so the REFLECTED INDEX of a pattern (t_1 ... t_k) on a row is
 *   refl(pos(0)) + N * (refl(pos(phi(t_1))) + N * (refl(pos(phi(t_2))) + ...))
 * with pos exactly the any-bytes rule above (the last position < N holding the byte, 0 if none): every digit is < N, so a
 * reflected look-up is in bounds for ANY bytes, like a plain one.  The reflected value of a row is
 *   max(sum_p table_p[index_p], sum_p table_p[reflected index_p]),
 * each sum over the whole set, 0xFE / 0xFF terms included: the larger of two admissible, consistent values, which is again
 * both.  A partition whose every pattern is its own mirror image (phi maps its tiles onto themselves) gains nothing:
 * the mirror is then an automorphism of each pattern's abstract graph, and the two look-ups read equal distances.
 * dca_pdb_eval_reflected: dca_pdb_eval with that value; the same parameters, the same refusals. */
int dca_pdb_eval_reflected(int dim, const uint8_t* states /*[n, ld]*/, int64_t n, int64_t ld, int num_patterns,
                           const uint8_t* tiles /*host*/, const int* ks /*host [num_patterns]*/,
                           const uint8_t* const* tables /*host [num_patterns] of device pointers*/, float* out /*[n]*/, void* stream);

/* Pattern databases for cube3 (csrc/dca_pdb_cube3.hip; `--env cube3 --model_dir pdb:<spec>`): Korf's distance tables over
 * corner cubies and over subsets of the edge cubies, combined by MAX (a face turn moves cubies of several patterns at once, so
 * the tables do not add).  Every table is admissible and consistent on its own, and so is their max.
 *   cubies       numbered from the move table (dca_cube3_perm_table): two sticker positions belong to one cubie exactly when the
 *                same set of the 12 moves displaces them — 8 classes of three (corners, kind DCA_CUBE3_CORNERS: n = 8 slots,
 *                o = 3 orientations), 12 of two (edges, DCA_CUBE3_EDGES: n = 12, o = 2), and the 6 centres.  A cubie's
 *                positions are listed in ascending order, the cubies of a kind are ordered by their smallest position, and slot
 *                s is the home of cubie s.  dca_cube3_pdb_cubies writes the lists, [n][o] position bytes (host).
 *   pattern      an ordered list of k distinct cubies of one kind, 1 <= k <= 8; its table is caller-owned device memory of
 *                dca_cube3_pdb_bytes(kind, k) = P(n, k) * o^k bytes, P(n, k) = n! / (n - k)! (a pure function; DCA_E_BADARG
 *                unless kind is 0 or 1, k is 1..8 and the result is <= 2^34: nine edges are refused).
 *   location     cubie j of a state is at (s_j, r_j): s_j = the slot that holds it, r_j = the index, within slot s_j's position
 *                list, of the position that shows the cubie's reference facelet — the facelet whose home is the cubie's
 *                smallest position.
 *   index rule   slot rank, most significant digit first: digit j is d_j = s_j - #{i < j : s_i < s_j} in radix n - j; then
 *                index = rank * o^k + the k orientation digits r_j in radix o, cubie 0 most significant.  The goal has every
 *                cubie at home with r = 0.  No special case for k = n: all eight corners take 8! * 3^8 bytes of which a third
 *                is reachable.
 *   value rule   table[index] = the breadth-first distance, in the 12-move metric, of the abstract state (the locations of the
 *                pattern's cubies, everything else invisible) to the goal; an entry no move sequence reaches holds 0xFE.
 * dca_cube3_pdb_build fills `table` level by level: sweep d gives the value d to every entry that is still 0xFE and has a
 * neighbour (one of the 12 moves away) at d - 1; one thread per entry pulls and writes only its own byte.  It SYNCHRONISES the
 * stream once per sweep to read a "filled" word.  *sweeps (host, or NULL) = the sweeps it took = the deepest level + 1, the
 * last, empty one included: the table AND the count are the same on every run.  cubies: host [k].
 * dca_cube3_pdb_index (host only, no device call) is the index of one 54-byte row by the code the kernels run.
 * dca_cube3_pdb_eval: out[i] = max over the patterns of table_p[index_p(row i)], an integer <= 255, exact in fp32.  states:
 * device rows [n, ld], ld >= 54, any byte alignment.  row_kind says what a row's bytes are: DCA_ROWS_STATE sticker ids 0..53
 * (turned into colours, id / 9, on load) or DCA_ROWS_NNET the 54 colour bytes 0..5 of the network input — what
 * dca_engine_pop_expand_packed and dca_engine_root_nnet_in hand a heuristic closure for cube3.  kinds, ks: host
 * [num_patterns]; cubies: host, the patterns' cubie lists one after another; tables: HOST array of num_patterns device
 * pointers.  Up to 24 patterns; patterns MAY share cubies (a max stays admissible); within a pattern the cubies are distinct.
 * The metadata travels as kernel arguments; stream-ordered, nothing synchronises.
 *   colour rule  a slot's cubie is recognised by the SET of colours on the slot's positions and oriented by where the smallest
 *                of them sits (a cubie's reference facelet has its smallest colour): r = the first position of the slot's list
 *                that holds the slot's smallest byte.
 *   any-bytes rule  the engine pads closure input to a multiple of 1024 rows whose padding is stale or zero, so every read is in
 *                bounds for ANY 54 bytes: a byte above 5 (after id / 9 for DCA_ROWS_STATE) belongs to no colour set; cubie j's
 *                location is that of the LAST slot whose colour set is the cubie's, (0, 0) if there is none; a rank digit is
 *                clamped to its radix, d_j <= n - j - 1.  Every index is then < P(n, k) * o^k by construction.  The value of a
 *                row that is no cube state is whatever the tables hold there, and is deterministic.
 * DCA_E_BADARG before any launch, the message naming the argument: kind outside {0, 1}; k outside 1..8 or a table over 2^34
 * bytes; a cubie >= n or named twice in its pattern; num_patterns outside 1..24; row_kind outside {0, 1}; a NULL cubies / kinds
 * / ks / tables / table / row / index / positions / out (states and out may be NULL when n == 0); out not 4-byte aligned;
 * ld < 54; n < 0 or >= 2^31. */
#define DCA_CUBE3_CORNERS 0
#define DCA_CUBE3_EDGES 1
#define DCA_ROWS_STATE 0
#define DCA_ROWS_NNET 1
int64_t dca_cube3_pdb_bytes(int kind, int k);
int dca_cube3_pdb_cubies(int kind, uint8_t* positions /*host [n*o]*/);
int dca_cube3_pdb_index(int kind, const uint8_t* cubies /*host [k]*/, int k, const uint8_t* row /*host [54]*/, int row_kind,
                        int64_t* index /*host*/);
int dca_cube3_pdb_build(int kind, const uint8_t* cubies /*host [k]*/, int k, uint8_t* table /*device [P(n,k)*o^k]*/,
                        int* sweeps /*host or NULL*/, void* stream);
int dca_cube3_pdb_eval(const uint8_t* states /*[n, ld]*/, int64_t n, int64_t ld, int row_kind, int num_patterns,
                       const int* kinds /*host [num_patterns]*/, const uint8_t* cubies /*host*/,
                       const int* ks /*host [num_patterns]*/, const uint8_t* const* tables /*host [num_patterns] of device pointers*/,
                       float* out /*[n]*/, void* stream);

/* Symmetric look-ups (`pdb:<spec>+sym`, `pdb:<spec>+sym:N`; cube3 only): every rotation and reflection sigma of the cube is an
 * automorphism of the move graph that fixes the goal, so d(s) = d(sigma s sigma^-1), and table_Q read at the conjugate of s is an
 * admissible bound on d(s) for every sigma — consistent too, because one move of s is one move of the conjugate.  The same
 * tables, read up to 48 times, no table bytes.  Everything below is derived from the move table, once, at first use; a
 * derivation that fails its own checks (every conjugated move is a move; the 48 move maps are distinct; no location map
 * contradicts itself) makes every symmetric entry point return DCA_E_STATE.
 *   symmetries   two faces (colours, position / 9) are opposite exactly when no cubie carries both: 0/1, 2/3, 4/5.  A symmetry is
 *                a face map phi, a permutation of the 6 faces with phi(opposite(f)) = opposite(phi(f)); there are 3! * 2^3 =
 *                DCA_CUBE3_SYMS = 48.  ORDER: ascending lexicographic order of (phi(0), phi(1), ..., phi(5)); symmetry 0 is the
 *                identity.  sigma, its sticker permutation, sends the position on face f of the cubie with colour set F to the
 *                position on face phi(f) of the cubie with colour set phi(F) (a centre: F = {f}).  pi, its move map, is the move
 *                with sigma o P_a o sigma^-1 = P_pi(a); as gather tables (dca_cube3_perm_table) perm[pi(a)][sigma(i)] =
 *                sigma(perm[a][i]).  24 symmetries keep a move's direction bit, the reflections flip it.  The conjugate S' of a
 *                row S of sticker ids is S'[sigma(p)] = sigma(S[p]); conjugation commutes with the moves through pi.
 *   look-up      for a pattern Q = (q_0 ... q_{k-1}) the table byte at the conjugated row needs no conjugated row: it is the
 *                table read at index rule(R_{sigma,c_0}[location(c_0)], ..., R_{sigma,c_{k-1}}[location(c_{k-1})]) with the
 *                SOURCE cubies c_j = sigma^-1(q_j) (sigma as a map of cubies, by colour sets) and the location maps R_{sigma,c},
 *                24 -> 24, fixed by R[home(c)] = home(sigma(c)) and R[move_a(l)] = move_pi(a)(R[l]).
 *   images       a pattern's images are its DISTINCT source cubie sets {c_j}, in the symmetries' order — the pattern itself
 *                (the identity) first.  Two symmetries with the same set read equal values; the first one stands for the set.
 *                max_images = N in 1..48 takes the first min(N, distinct) images of EACH pattern; 48 takes all.  The look-up
 *                list is pattern 0's images, then pattern 1's, ...  A list of more than DCA_CUBE3_SYM_MAX_LOOKUPS = 64 look-ups
 *                is refused, the message naming the cap and `+sym:N`.  Six- and seven-edge patterns have 24 images, all eight
 *                corners one: `korf` and `korf7` with every image are 1 + 24 + 24 = 49 look-ups.
 *   value        the largest table byte over the list.  max_images = 1 is dca_cube3_pdb_eval's value, bit for bit; the value
 *                never decreases with max_images.  The any-bytes rule holds as above: a location is < 24 whatever the row's
 *                bytes are, so every map read is inside its 24-byte row, a mapped location is < 24, and the rank clamps its
 *                digits.
 * dca_cube3_pdb_eval_sym: dca_cube3_pdb_eval with that value; the same parameters and refusals, plus max_images outside 1..48
 * and the cap.  The list (13.8 KB) is kept in device memory by the library: the FIRST call with a new pattern set or new table
 * addresses allocates and copies it (hipMalloc, hipMemcpy: blocking the host, and NOT allowed under a stream capture — make
 * a set's first call before capturing); later calls make no HIP call but the launch.  The library keeps eight lists per
 * entry-point family and frees the oldest for a ninth (hipFree: waits for the device, not allowed under a capture either);
 * more than eight distinct (set, tables) combinations in use by concurrent host threads are not supported. */
#define DCA_CUBE3_SYMS 48
#define DCA_CUBE3_SYM_MAX_LOOKUPS 64
int dca_cube3_pdb_eval_sym(const uint8_t* states /*[n, ld]*/, int64_t n, int64_t ld, int row_kind, int num_patterns,
                           const int* kinds /*host [num_patterns]*/, const uint8_t* cubies /*host*/,
                           const int* ks /*host [num_patterns]*/, const uint8_t* const* tables /*host [num_patterns] of device pointers*/,
                           int max_images, float* out /*[n]*/, void* stream);

/* Dual look-ups (`pdb:<spec>+dual`, `pdb:<spec>+sym:N+dual`; cube3 only; Zahavi, Felner, Holte, Schaeffer 2008, "Duality in
 * permutation state spaces"): the 12 moves are closed under inversion (a ^ 1), so if s = m_1 ... m_d then s^-1 = m_d^-1 ... m_1^-1
 * and d(s^-1) = d(s): any table read at the INVERSE state is an admissible bound on d(s).  The pattern's cubies sit elsewhere in
 * s^-1, so the byte usually differs from the one at s.  The inverse of a conjugate is the conjugate of the inverse, so every
 * entry of the symmetric look-up list can be read a second time at the inverse: the same tables, the same list, no table bytes.
 *   inverse row  for a row S of sticker ids that is a cube state, S^-1[S[p]] = p (numpy: argsort(S)).
 *   dual value   of S under (pattern set, max_images = N): max(v(S), v(S^-1)), v = the value of dca_cube3_pdb_eval_sym at N
 *                (N = 1: the plain max over the patterns).  Never below v(S); never above d(S).
 *   in location words   no kernel builds S^-1: the inverse is taken in cubie coordinates, on the two words of the colour rule
 *                (5 bits a cubie, location = slot * o + r).  INVERSION RULE: start from the all-zero word; for cubie
 *                j = 0 ... n-1 in ascending order at location (s_j, r_j), REPLACE field s_j by the location (j, r'_j).  The
 *                orientation: r' = r for an edge.  The corner slots fall into two classes of four (the ascending positions of a
 *                slot run clockwise round one class and anticlockwise round the other; read off the move table: a quarter turn
 *                carries a slot's positions x -> x + c onto its own class, x -> c - x onto the other); r' = (3 - r) mod 3
 *                where slot s_j and slot j are of one class, r' = r where they are not.  On every cube state the result is
 *                the location words of argsort(S).  A row of colours (DCA_ROWS_NNET) goes through the colour rule first, as
 *                everywhere, and its words are inverted by the same rule.
 *   replacing rule   a field is replaced (mask, then or), never or-ed onto stale bits: the last writer wins, a slot that no
 *                cubie names keeps location 0.  Every inverted location is therefore < 24 for ANY 54 bytes, and every map
 *                read and every rank stays in bounds as above (the any-bytes rule).  The IDA* lane uses the or-only form —
 *                the same words wherever the n slots of a kind are distinct — which its root is checked for and the moves keep.
 *   k = n skip   a pattern that names all n cubies of its kind (the 8-corner table) abstracts nothing of that kind: its byte
 *                is the distance in the group of that kind's cubies, where d(s^-1) = d(s) too, so its dual byte equals its
 *                regular byte on every cube state.  Its dual look-ups are skipped: they count 0 in the second pass, on ANY
 *                bytes.
 *   order        the whole look-up list is read at the state first, then again at the inverted words (the look-ups that are
 *                not skipped, in the list's order).  A search computes the inverted words only where the first pass has not
 *                already pruned the child.
 * dca_cube3_pdb_eval_dual: dca_cube3_pdb_eval_sym with that value: its parameters, its refusals, its list (unchanged, the cap
 * stays DCA_CUBE3_SYM_MAX_LOOKUPS list entries) and the library's device copies of it. */
int dca_cube3_pdb_eval_dual(const uint8_t* states /*[n, ld]*/, int64_t n, int64_t ld, int row_kind, int num_patterns,
                            const int* kinds /*host [num_patterns]*/, const uint8_t* cubies /*host*/,
                            const int* ks /*host [num_patterns]*/, const uint8_t* const* tables /*host [num_patterns] of device pointers*/,
                            int max_images, float* out /*[n]*/, void* stream);

/* Exact LightsOut heuristic (csrc/dca_lightsout_exact.hip; `--env lightsout7 --model_dir exact:gf2`): the true distance of any
 * state, by linear algebra over GF(2) instead of a table.
 *   algebra      pressing cell a flips a fixed set of cells, presses commute, and pressing a cell twice is the identity.  A
 *                state is therefore s = A x (mod 2), x = the cells pressed an odd number of times, A[i][a] = 1 where a press
 *                of a flips cell i (the move matrix of lights_out.py:33-44; A is symmetric).  On the 7 x 7 board A has rank 49:
 *                x = A^-1 s is the only press set that makes s, pressing its cells once each, in any order, is the shortest
 *                solution, and the distance is popcount(A^-1 s).  A^-1 is derived at compile time from the move rule; a board
 *                size whose matrix is singular (4 x 4, 5 x 5) does not compile.
 *   bit-0 rule   cell i of a row contributes bit 0 of its byte, b & 1.  The engine pads closure input to a multiple of 1024
 *                rows whose padding is stale or zero: no byte forms an address, so ANY bytes are in bounds, and a row's value is
 *                that of the same row reduced to b & 1 (the any-bytes rule).
 * dca_lightsout_exact_matrix (host only, no device call): rows[a] = row a of A^-1 as the kernels use it, bit i for cell i, bits
 * 49..63 zero.
 * dca_lightsout_exact_eval: out[i] = popcount(A^-1 row_i), an integer <= 49, exact in fp32.  dca_lightsout_exact_solve:
 * presses[i] has bit a set iff cell a is in the optimal solution of row i; popcount(presses[i]) is eval's out[i].  states:
 * device rows [n, ld], ld >= 49, any byte alignment (word loads when the base pointer and ld are both multiples of 4, byte loads
 * otherwise).  Stream-ordered, nothing synchronises.
 * DCA_E_BADARG before any HIP call, the message naming the argument: dim other than 7; a NULL rows; n < 0 or >= 2^31; ld < 49;
 * a NULL states / out / presses when n > 0 (both may be NULL when n == 0, which launches nothing); out not 4-byte, presses not
 * 8-byte aligned. */
int dca_lightsout_exact_matrix(int dim, uint64_t* rows /*host [dim*dim]*/);
int dca_lightsout_exact_eval(int dim, const uint8_t* states /*[n, ld]*/, int64_t n, int64_t ld, float* out /*[n]*/, void* stream);
int dca_lightsout_exact_solve(int dim, const uint8_t* states /*[n, ld]*/, int64_t n, int64_t ld, uint64_t* presses /*[n]*/,
                              void* stream);

/* IDA* on the pattern databases (csrc/dca_idastar.hip; `python -m deepcubea_amd.search_methods.idastar`): iterative-deepening A*
 * (Korf 1985 / 1997), the search the tables were invented for.  No OPEN, no CLOSED, no node pool: memory is the caller's tables
 * plus a packed move stack per lane, so a search runs as long as its node budget lets it.  With an admissible table set the
 * solution it returns is optimal.  dim 3..5 for the puzzles (6 and 7 are refused: their optimal solutions are out of reach).
 *   inputs       root: HOST bytes, the N tiles of a board or the 54 sticker ids of a cube.  The pattern set exactly as
 *                dca_pdb_eval / dca_cube3_pdb_eval take it (host ids, ks, kinds; a HOST array of device table pointers); the
 *                puzzles take at most 8 patterns (a lane keeps one running index per pattern in registers), cube3 up to 24.
 *   thresholds   T_0 = h(root); the next T is the smallest f = g + h above T among the children generated.  One launch per
 *                threshold; the call SYNCHRONISES the stream after each to read the counters back.
 *   pruning      a child is generated unless its move a, after the previous move m (and m_prev before that), is:
 *                puzzles — a no-op (the blank at the board's edge), or a == m ^ 1;
 *                cube3, a = 2 face + dir, faces U D L R B F, f ^ 1 the opposite face — a == m ^ 1; a == m with a odd (a half
 *                turn is written with the even action only); a == m == m_prev; face(a) == face(m) ^ 1 with face(a) < face(m)
 *                (opposite faces commute: ascending order only).
 *   node count   every generated child (one that passes the pruning rules and whose h is evaluated) counts once.  A completed
 *                iteration's count is the same on every run; the last iteration ends early when a lane reaches the goal, so
 *                its count varies.  nodes_per_threshold[i] goes with thresholds[i]; *total_nodes is their sum.
 *   status       DCA_IDASTAR_SOLVED: *length moves, the first min(*length, moves_cap) of them in moves[] (a move is the
 *                environment's action number); applying them to the root gives the goal — for cube3 every cubie at home, not
 *                merely h = 0.  DCA_IDASTAR_BUDGET: the count passed max_nodes.  A lane adds its nodes to the launch's counter
 *                and polls the stop word every `interval` nodes, and a lane without an item counts nothing, so a launch counts at
 *                most (what was left of max_nodes) + min(items, lanes) * interval, and *total_nodes <= max_nodes + that product
 *                for the last launch.  `items` and `lanes` are those of "work items" below; interval =
 *                DCA_IDASTAR_POLL_NODES, or (what was left of max_nodes) / (2 lanes), at least 1, where that is smaller.  Whatever
 *                the launch: *total_nodes <= max_nodes + DCA_IDASTAR_MAX_LANES * DCA_IDASTAR_POLL_NODES and <= max_nodes +
 *                max(max_nodes / 2, DCA_IDASTAR_MAX_LANES).  A budget that ends inside the iteration that reaches the goal may still end
 *                solved, within these bounds.  DCA_IDASTAR_UNSOLVABLE: a table byte at the root is 0xFE or
 *                0xFF, the threshold passed DCA_IDASTAR_MAX_MOVES, or no child was left above the threshold.  All three return 0.
 *   work items   an iteration is split into items = NM * RADIX^(P - 1) move prefixes of depth P (one item, P = 0, in the first
 *                iterations), P the deepest the family finds worth it after a previous iteration of `prev` nodes (0 before the
 *                first): cube3 — NM = RADIX = 12, P <= 6, 12^P * P <= prev / 2; puzzles — NM = 4, RADIX = 3, P <= 15,
 *                4 * 3^(P - 1) <= 8 prev.  The launch has lanes = 256 * min(ceil(items / 256), 8 * compute units,
 *                DCA_IDASTAR_MAX_LANES / 256).  Results and completed iterations' counts do not depend on the split.
 *   capacities   *num_thresholds = the thresholds run; the first min(that, thresholds_cap) entries of thresholds[] and
 *                nodes_per_threshold[] are written.  A root that is the goal: solved, length 0, no threshold run.
 * DCA_E_BADARG before any HIP call, the message naming the argument: dim outside 3..5; a NULL root / ids / ks / kinds / tables /
 * table / status / length / num_thresholds / total_nodes, or a NULL buffer with a positive capacity; a negative capacity;
 * max_nodes <= 0; num_patterns outside 1..8 (puzzles) or 1..24 (cube3); what dca_pdb_eval / dca_cube3_pdb_eval refuse in a
 * pattern set; a puzzle root with a byte >= N, a tile twice, or the wrong parity (the goal cannot be reached from it); a cube3
 * root that is not the ids 0..53 once each. */
#define DCA_IDASTAR_SOLVED 0
#define DCA_IDASTAR_BUDGET 1
#define DCA_IDASTAR_UNSOLVABLE 2
#define DCA_IDASTAR_POLL_NODES 512
#define DCA_IDASTAR_MAX_LANES (1 << 19)
#define DCA_IDASTAR_MAX_MOVES 254
int dca_idastar_npuzzle(int dim, const uint8_t* root /*host [N]*/, int num_patterns, const uint8_t* tiles /*host*/,
                        const int* ks /*host [num_patterns]*/, const uint8_t* const* tables /*host [num_patterns] of device pointers*/,
                        int64_t max_nodes, int* status, int* length, uint8_t* moves /*host [moves_cap]*/, int moves_cap,
                        int* num_thresholds, int* thresholds /*host [thresholds_cap]*/,
                        int64_t* nodes_per_threshold /*host [thresholds_cap]*/, int thresholds_cap, int64_t* total_nodes, void* stream);
/* dca_idastar_npuzzle with h = the reflected value ("Reflected look-up" above).  A lane keeps a second running index per
 * pattern, that of the state's mirror image: a move of tile t from position nb to the blank's position b adds
 * w(t) * (b - nb) to the index of t's pattern, as in the plain search, and w(phi(t)) * (refl(b) - refl(nb)) to the reflected
 * index of phi(t)'s pattern (nothing where phi(t) is in no pattern); the blank digits b and refl(b) are added at the gather.
 * The root is unsolvable if any of the 2 * num_patterns root bytes is 0xFE or 0xFF.  Same parameters, outputs and refusals,
 * except that num_patterns must be in 1..4: the two indices per pattern share the 8 a lane keeps in registers. */
int dca_idastar_npuzzle_reflected(int dim, const uint8_t* root /*host [N]*/, int num_patterns, const uint8_t* tiles /*host*/,
                                  const int* ks /*host [num_patterns]*/,
                                  const uint8_t* const* tables /*host [num_patterns] of device pointers*/, int64_t max_nodes, int* status,
                                  int* length, uint8_t* moves /*host [moves_cap]*/, int moves_cap, int* num_thresholds,
                                  int* thresholds /*host [thresholds_cap]*/, int64_t* nodes_per_threshold /*host [thresholds_cap]*/,
                                  int thresholds_cap, int64_t* total_nodes, void* stream);
/* A batch of sliding-puzzle roots on one pattern set, searched in rounds: one launch runs the next threshold of every root
 * still searching, each root on its own blocks with its own counters, so that a states file's independent roots fill the chip
 * that one small search cannot.  roots: n_roots boards of N bytes; reflect != 0: the reflected search.  Every output is an
 * array, root r's at index r (moves: r * moves_cap, thresholds and nodes_per_threshold: r * thresholds_cap).
 * The contract: root r's outputs are those of dca_idastar_npuzzle (or dca_idastar_npuzzle_reflected where reflect != 0) called
 * on that root alone with the same max_nodes: the status, the length, a move list that solves the root at that length (it need
 * not be the same list), the thresholds and every completed threshold's count; the last threshold's count varies, as it does
 * there.  max_nodes is per root and the budget bounds are the single search's, per root: root r's launch of a round has
 * the blocks, lanes, items and interval of "work items" and "status" above, from that root's own previous count.  One root's
 * budget or solution does not end another's search: a root that is solved, out of budget, unsolvable, dead at the root or
 * already the goal leaves the batch, and the call ends with the round that has no root left.
 * Per round the call SYNCHRONISES the stream once; the control blocks and the root descriptors are allocated once per call.
 * DCA_E_BADARG before any HIP call and with no output written: what dca_idastar_npuzzle refuses (reflect: num_patterns in
 * 1..4), n_roots outside 1..DCA_IDASTAR_MAX_BATCH, and a bad root, which the message names by its index ("roots[i]: tile 3
 * appears twice", "roots[i]: ... the wrong parity"): the whole call is refused. */
#define DCA_IDASTAR_MAX_BATCH 1024
int dca_idastar_npuzzle_batch(int dim, const uint8_t* roots /*host [n_roots, N]*/, int n_roots, int num_patterns,
                              const uint8_t* tiles /*host*/, const int* ks /*host [num_patterns]*/,
                              const uint8_t* const* tables /*host [num_patterns] of device pointers*/, int reflect,
                              int64_t max_nodes /*per root*/, int* status /*[n_roots]*/, int* length /*[n_roots]*/,
                              uint8_t* moves /*[n_roots, moves_cap]*/, int moves_cap, int* num_thresholds /*[n_roots]*/,
                              int* thresholds /*[n_roots, thresholds_cap]*/, int64_t* nodes_per_threshold /*[n_roots, thresholds_cap]*/,
                              int thresholds_cap, int64_t* total_nodes /*[n_roots]*/, void* stream);
int dca_idastar_cube3(const uint8_t* root /*host [54]*/, int num_patterns, const int* kinds /*host [num_patterns]*/,
                      const uint8_t* cubies /*host*/, const int* ks /*host [num_patterns]*/,
                      const uint8_t* const* tables /*host [num_patterns] of device pointers*/, int64_t max_nodes, int* status, int* length,
                      uint8_t* moves /*host [moves_cap]*/, int moves_cap, int* num_thresholds, int* thresholds /*host [thresholds_cap]*/,
                      int64_t* nodes_per_threshold /*host [thresholds_cap]*/, int thresholds_cap, int64_t* total_nodes, void* stream);
/* dca_idastar_cube3 on the symmetric look-ups ("Symmetric look-ups" above): h = the largest byte over the look-up list of
 * (pattern set, max_images).  Same state, moves, pruning rules, work items, counting, budget and ending.  The root is
 * unsolvable if ANY look-up's byte at the root is 0xFE or 0xFF.  A lane may stop reading the list at the first value v with
 * g + 1 + v > T: the child is pruned exactly when it is under the full maximum, but the f it records for the next threshold may
 * then be smaller than its exact f.  The contract, whatever the evaluation order:
 *   - the thresholds increase strictly; the first is h(root) over all look-ups, the last of a solved search the solution length;
 *   - every threshold of the exact search (h = the full maximum everywhere) occurs among them;
 *   - a completed threshold's node count is that of the tree at that threshold under the full maximum: a property of the
 *     tree, not of the schedule, the split into work items or the order of the look-ups.
 * Same parameters, outputs and refusals as dca_idastar_cube3, plus max_images outside 1..48 and a list over
 * DCA_CUBE3_SYM_MAX_LOOKUPS.  max_images = 1 runs dca_idastar_cube3's thresholds and completed counts. */
int dca_idastar_cube3_sym(const uint8_t* root /*host [54]*/, int num_patterns, const int* kinds /*host [num_patterns]*/,
                          const uint8_t* cubies /*host*/, const int* ks /*host [num_patterns]*/,
                          const uint8_t* const* tables /*host [num_patterns] of device pointers*/, int max_images, int64_t max_nodes,
                          int* status, int* length, uint8_t* moves /*host [moves_cap]*/, int moves_cap, int* num_thresholds,
                          int* thresholds /*host [thresholds_cap]*/, int64_t* nodes_per_threshold /*host [thresholds_cap]*/,
                          int thresholds_cap, int64_t* total_nodes, void* stream);
/* dca_idastar_cube3_sym on the dual look-ups ("Dual look-ups" above): h = the dual value of (pattern set, max_images).  The
 * heuristic is admissible but not consistent (a move can change the byte at the inverse state by more than 1); IDA* needs only
 * admissibility, and the first solution found is optimal.  No bidirectional pathmax.  Same state, moves, pruning rules, work
 * items, counting, budget and ending; the inverse is not kept in a lane's state but made from the child's two words, in
 * registers, where the first pass does not prune the child.  h(root) is computed on the host in full: the root is unsolvable
 * if ANY regular or dual byte at the root is 0xFE or 0xFF.  Both passes may stop at the first value v with g + 1 + v > T.  The
 * contract, whatever the evaluation order:
 *   - the thresholds increase strictly; the first is h(root) over all regular and dual look-ups, the last of a solved search the
 *     solution length;
 *   - every threshold of the exact search (h = the full dual value everywhere) occurs among them;
 *   - a completed threshold's node count is that of the tree at that threshold under the full dual value: a property of the
 *     tree — and never more than the count of dca_idastar_cube3_sym at the same max_images and threshold, whose tree contains it.
 * Same parameters, outputs and refusals as dca_idastar_cube3_sym, and one more: a root whose 54 distinct sticker ids put two
 * cubies of a kind into one slot (no cube state: no move sequence solves it) is DCA_E_BADARG, "root: ...". */
int dca_idastar_cube3_dual(const uint8_t* root /*host [54]*/, int num_patterns, const int* kinds /*host [num_patterns]*/,
                           const uint8_t* cubies /*host*/, const int* ks /*host [num_patterns]*/,
                           const uint8_t* const* tables /*host [num_patterns] of device pointers*/, int max_images, int64_t max_nodes,
                           int* status, int* length, uint8_t* moves /*host [moves_cap]*/, int moves_cap, int* num_thresholds,
                           int* thresholds /*host [thresholds_cap]*/, int64_t* nodes_per_threshold /*host [thresholds_cap]*/,
                           int thresholds_cap, int64_t* total_nodes, void* stream);
/* Bounded batches: many cube3 roots on one pattern set and look-up mode, searched in the rounds of dca_idastar_npuzzle_batch —
 * one launch runs the next threshold of every root still searching, root r on the blocks its single search would get and with
 * its own control block.  For SHALLOW roots with a bound on the length, such as the windows of a found solution
 * (search_methods/refine.py); a shipped state fills the chip by itself and gains nothing here.  roots: n_roots cubes of 54
 * sticker ids.  max_images = 0 and dual = 0: the search of dca_idastar_cube3; max_images in 1..48: that of
 * dca_idastar_cube3_sym, or, where dual != 0, of dca_idastar_cube3_dual (dual != 0 with max_images = 0 is refused, as
 * max_images).  Every output is an array, root r's at index r, as dca_idastar_npuzzle_batch lays them out.
 * The contract: root r's status, length, thresholds and completed counts are those of the matching single entry point called on
 * that root alone with the same max_nodes (a move list that solves the root at that length; the last threshold's count
 * varies, as it does there).  max_length[r] = B changes one thing: a root whose next threshold would exceed B — h(root)
 * included, in which case nothing is launched for it — stops with status DCA_IDASTAR_BOUNDED, "no solution of at most B
 * moves": with an admissible set the thresholds run are the single search's thresholds <= B, with their counts, and no
 * threshold above B is among them.  max_length = NULL, or B >= DCA_IDASTAR_MAX_MOVES: no bound.  max_nodes is per root and
 * the budget bounds are the single search's, per root; one root's budget, bound or solution does not end another's search.
 * Per round the call does one memset, one upload, one launch and one read-back and SYNCHRONISES the stream once; the look-up
 * list's device copy is made (or found) once per call, the control blocks and descriptors are allocated once per call.
 * DCA_E_BADARG before any HIP call and with no output written: what the matching single entry point refuses, n_roots outside
 * 1..DCA_IDASTAR_MAX_BATCH, a negative max_length[i], and a bad root, which the message names by its index ("roots[i]: ...",
 * the dual search's "no cube state" included): the whole call is refused. */
#define DCA_IDASTAR_BOUNDED 3
int dca_idastar_cube3_batch(const uint8_t* roots /*host [n_roots, 54]*/, int n_roots, int num_patterns,
                            const int* kinds /*host [num_patterns]*/, const uint8_t* cubies /*host*/, const int* ks /*host [num_patterns]*/,
                            const uint8_t* const* tables /*host [num_patterns] of device pointers*/, int max_images /*0: plain*/, int dual,
                            const int* max_length /*host [n_roots] or NULL*/, int64_t max_nodes /*per root*/, int* status /*[n_roots]*/,
                            int* length /*[n_roots]*/, uint8_t* moves /*[n_roots, moves_cap]*/, int moves_cap,
                            int* num_thresholds /*[n_roots]*/, int* thresholds /*[n_roots, thresholds_cap]*/,
                            int64_t* nodes_per_threshold /*[n_roots, thresholds_cap]*/, int thresholds_cap,
                            int64_t* total_nodes /*[n_roots]*/, void* stream);

/* state hash (a9). The reference's hash VALUES are process-randomised SipHash (cube3.py:17-21)
 * or unpinned boost::hash_range (parallel_weighted_astar.cpp:104-111); what is pinned is key
 * equality.  This library defines, for a D-byte state split in little-endian 8-byte words
 * w_0..w_{ceil(D/8)-1} (last word zero-padded):
 *     h = 0x9E3779B97F4A7C15 ^ (D * 0xD6E8FEB86659FD93)
 *     for k: h ^= w_k; h *= 0xFF51AFD7ED558CCD; h ^= h >> 32
 *     h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53; h ^= h >> 33
 * The HIP kernels and the CPU oracle are bit-exact on it.                                    */

/* ---- a10-a13: device-resident BWAS engine ----------------------------------------------
 * Replaces cpp/parallel_weighted_astar.cpp (argv/stdout/socket) and the Instance/AStar
 * bookkeeping of search_methods/astar.py:50-90,232-340.  One engine = one search instance
 * on the current device.  OPEN, CLOSED and the node pool live in HBM; the heuristic is
 * supplied between the two halves of an iteration:
 *
 *     dca_engine_reset(e, root)
 *     dca_engine_root_commit(e, h_root)                        (PY semantics only)
 *     loop:  dca_engine_pop_expand(e, &nnet_in, &onehot, &m)  ->  h = heuristic(nnet_in[m])
 *            dca_engine_commit(e, h)
 *            dca_engine_status(e, &st);  stop when st.done
 *     dca_engine_solution(e, moves, &len, &path_cost)
 */
typedef struct dca_engine dca_engine;

typedef struct dca_status {
    int32_t done;            /* search finished (goal popped / cpp stop rule hit)            */
    int32_t failed;          /* capacity exhausted or OPEN ran empty                          */
    int64_t iterations;      /* completed pop/expand/commit iterations                        */
    int64_t nodes_generated; /* reference's "# Nodes Gen" (astar.py:168 / cpp:166,266)        */
    int64_t nodes_expanded;  /* parents popped and expanded                                   */
    int64_t open_size;
    int64_t closed_size;
    int64_t pool_size;       /* node ids handed out                                           */
    double best_cost;        /* cost of the cheapest solved node popped so far (cpp) / NaN    */
} dca_status;

/* onehot_dtype: DCA_DT_* to have pop_expand also emit the one-hot rows of the batch's children
 * (fused into the expansion launch), or -1 for none.  max_nodes bounds the node pool (one id per
 * generated child), the CLOSED table (2x, power of two) and OPEN.                                 */
int dca_engine_create(dca_engine** out, int env, int dim, double weight, int batch_size,
                      int64_t max_nodes, int semantics, int onehot_dtype);
/* K independent search instances of the same geometry in ONE engine: every kernel is launched once for all of
 * them (grid.y = instance), the way the reference's AStar steps a list of instances together
 * (astar.py:232-317).  A batch-20 000 iteration is launch/latency bound, so K scrambles advance in little more
 * than the time of one.  Instances are inert until reset with a root; each has its own OPEN/CLOSED/pool
 * (max_nodes each).  The un-suffixed calls below act on instance 0; pop_expand/commit/run_builtin act on all. */
int dca_engine_create_multi(dca_engine** out, int env, int dim, double weight, int batch_size,
                            int64_t max_nodes, int semantics, int onehot_dtype, int num_instances /*1..64*/);
int dca_engine_num_instances(dca_engine* e);
void dca_engine_destroy(dca_engine* e);
int dca_engine_reset(dca_engine* e, const uint8_t* root /*host [D]*/, void* stream);
int dca_engine_reset_instance(dca_engine* e, int inst, const uint8_t* root /*host [D]*/, void* stream);
/* PY semantics: cost(root) = w*0 + max(h,0)*!solved (astar.py:244-249). h_root: device f32[1].
 * CPP semantics never evaluates the root (cpp:160) — the call is then a no-op.                    */
int dca_engine_root_commit(dca_engine* e, const float* h_root, void* stream);
int dca_engine_root_commit_instance(dca_engine* e, int inst, const float* h_root, void* stream);
/* network-input row of the root (device [D]; cube3: colour index), valid after reset            */
int dca_engine_root_nnet_in(dca_engine* e, const uint8_t** nnet_in);
int dca_engine_root_nnet_in_instance(dca_engine* e, int inst, const uint8_t** nnet_in);
/* first half: pop min(B,|OPEN|) by (cost, push order), expand.  *nnet_in = device pointer to the
 * network-input rows [K*batch*num_moves, D] (instance-major) of the batch's children (cube3: colour index; puzzles:
 * the tiles), child index = pop_rank*num_moves + move; *onehot = their one-hot rows
 * [K*batch*num_moves, D*depth] (NULL unless enabled at create).  Both buffers have the FIXED row
 * count m_capacity = K*batch*num_moves so the heuristic can be enqueued without a host sync; rows
 * past the live child count hold stale but valid rows and their heuristic values are ignored.     */
int dca_engine_pop_expand(dca_engine* e, const uint8_t** nnet_in, const void** onehot,
                          int64_t* m_capacity, void* stream);
/* second half: h = device f32[m_capacity].  max(h,0) is applied here (nnet_utils.py:193-194
 * clip_zero=True): cost, CLOSED dedup, push.                                                      */
int dca_engine_commit(dca_engine* e, const float* h, void* stream);
/* Dedup-first ("packed") stepping.  The reference runs the network on every child and only then drops the
 * children already in CLOSED (astar.py:272-282 "do heur before check"); a dropped child's value is never used, so
 * checking first and evaluating only the survivors gives the identical search with ~15 % (cube3) to ~40 %
 * (sliding puzzles) fewer network rows, and none at all for the padding rows of a short batch.
 *   enable_packed    once after create: allocates the packed batch buffers.  onehot_dtype DCA_DT_* / -1;
 *                    onehot_row_stride >= D*depth elements with stride*sizeof(elt) a multiple of 16 (rows are
 *                    written with a zero tail so a GEMM can use the padded K directly).
 *   pop_expand_packed  pop, expand, CLOSED check, pack.  *rows = kept children of all instances this iteration
 *                    (synchronises to return it); *nnet_in [rows, D], *onehot [rows, stride], *src [rows] =
 *                    instance*batch*num_moves + child index of each packed row.  The buffers are sized to
 *                    K*batch*num_moves rounded up to 1024 rows; rows past *rows hold stale but finite data.
 *   commit_packed    h = device f32[rows] in packed row order: cost and push of the kept children.        */
int dca_engine_enable_packed(dca_engine* e, int onehot_dtype, int64_t onehot_row_stride);
int dca_engine_pop_expand_packed(dca_engine* e, const uint8_t** nnet_in, const void** onehot, const uint32_t** src,
                                 int64_t* rows, void* stream);
int dca_engine_commit_packed(dca_engine* e, const float* h, void* stream);
/* what the last pop_expand_packed found besides its row count (no extra sync: read with it): how many of the engine's
 * instances were already finished when it ran (done: goal popped and accepted, OPEN empty, or failed) and how many of those
 * failed (node pool exhausted, ...).  A host loop stops stepping when instances_done == K instead of polling the status. */
int dca_engine_packed_state(dca_engine* e, int* instances_done, int* instances_failed);
/* both halves with a built-in heuristic (evaluated inside the expansion launch), `iters`
 * iterations enqueued without any host sync (kernels no-op once the search is done).
 * use_graph != 0 replays one captured hipGraph per iteration instead of eager launches.           */
int dca_engine_run_builtin(dca_engine* e, int heur_id, int iters, int use_graph, void* stream);
/* synchronises the stream */
int dca_engine_status(dca_engine* e, dca_status* out, void* stream);
int dca_engine_status_instance(dca_engine* e, int inst, dca_status* out, void* stream);
/* ASTAR updates (updaters/updater.py:36-54 of the reference: one batch-1 search per training state, each with its own random
 * weight, stepped together; every popped node becomes a training target).
 *   set_weight_instance  weight of path cost of one instance (astar.py:196 `weights`), between iterations; set_weights: of the
 *                        first n instances at once (one synchronisation);
 *   park_instance        marks an instance finished (its launches become no-ops) until its next reset; between iterations
 *                        only (DCA_E_STATE between pop_expand and commit: the commit half records the CLOSED slots the
 *                        expansion half claimed);
 *   last_popped          between pop_expand and commit: the parents of this pop, instance-major — states device u8
 *                        [K*batch, D], flags device u8 [K*batch]: 0 = nothing popped in that slot, 1 = popped, 2 = popped and
 *                        solved (Node.is_solved: its backup is 0, astar.py:38-40). */
int dca_engine_set_weight_instance(dca_engine* e, int inst, double weight);
int dca_engine_set_weights(dca_engine* e, const double* weights /*host [n], instances 0..n-1*/, int n);
int dca_engine_park_instance(dca_engine* e, int inst, void* stream);
int dca_engine_last_popped(dca_engine* e, uint8_t* states, uint8_t* flags, void* stream);
/* The same controls without a host round trip, for stepping thousands of batch-1 searches (one ASTAR update = up to 5e5 of
 * them, updater.py:36-54): everything is enqueued on `stream`, nothing synchronises.
 *   reset_many        instances 0..n-1 restart from roots_dev (device u8 [n, D]; NOT range-checked — the rows come from the
 *                     library's own generator), instances n..K-1 are parked;
 *   root_commit_many  h_roots_dev: device float [n], the heuristic of the n roots;
 *   set_weights_dev   weights of path cost of instances 0..n-1 from a device double [n] (stream-ordered, nothing
 *                     synchronises); they hold until a host-side dca_engine_set_weights / dca_engine_set_weight_instance
 *                     names the same instance: every call that re-uploads the host's copy of the instance table (set_tiers,
 *                     the profile calls, the host setters) first reads the device's weights back into it.  A weight < 0 or
 *                     NaN — which the host setters refuse with DCA_E_BADARG — is clamped to 0 by the launch. */
int dca_engine_reset_many(dca_engine* e, const uint8_t* roots_dev, int n, void* stream);
int dca_engine_root_commit_many(dca_engine* e, const float* h_roots_dev, int n, void* stream);
int dca_engine_set_weights_dev(dca_engine* e, const double* weights_dev, int n, void* stream);
/* facts about an engine (host int64[8]): [0] workgroups of k_sel_collect's grid, [1] how many of them the device holds at once
 * according to hipOccupancyMaxActiveBlocksPerMultiprocessor (-1: query failed), [2] 1 if the grid-wide refinement of giant tie
 * bins (grid barriers; needs [1] >= [0]) was enabled at creation, [3] bytes of the CLOSED table, [4] 1 once a grid barrier
 * found the launch not fully resident (the GPU is shared) and the engine fell back to the single-workgroup path for good;
 * [5..7] reserved.  Synchronises.  (knob 10 of dca_debug_tune makes the first barrier of every giant iteration give up at
 * once: the test hook for that fallback.) */
int dca_engine_info(dca_engine* e, int64_t* out /*host [8]*/, void* stream);
/* child rows of the last pop_expand straight from the node pool (device [m_live, D]); synchronises */
int dca_engine_last_children(dca_engine* e, const uint8_t** states, int64_t* m_live, void* stream);
/* root->goal move list (astar.py:213-229 get_path / cpp:336-341).  synchronises.                 */
int dca_engine_solution(dca_engine* e, int32_t* moves /*host [cap]*/, int cap, int* len, double* path_cost, void* stream);
int dca_engine_solution_instance(dca_engine* e, int inst, int32_t* moves /*host [cap]*/, int cap, int* len,
                                 double* path_cost, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training step: BatchNorm1d in training mode over row-major [n, c] float32 activations, as
 * nn.BatchNorm1d runs inside nnet_utils.train_nnet (utils/nnet_utils.py:53-118, utils/pytorch_models.py:57-86),
 * optionally fused with the residual add and the ReLU that follow it in the network:
 *   forward   y = relu?( (x - mean_c) * invstd_c * gamma_c + beta_c (+ skip) ), batch statistics over the n rows
 *             (biased variance normalises; var_unbiased feeds running_var, momentum is the caller's business)
 *   backward  g = dy * (y > 0 if relu); dbeta = sum g; dgamma = sum g*xhat;
 *             dx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n); dskip = g (if dskip != NULL)
 * Column sums are accumulated in fp64 and folded deterministically.  workspace: dca_bn_workspace_bytes(c) bytes.
 * ------------------------------------------------------------------------------------------------------------------ */
int64_t dca_bn_workspace_bytes(int64_t c);
int dca_bn_train_forward(const float* x, const float* skip /*or NULL*/, const float* gamma, const float* beta, int64_t n,
                         int64_t c, double eps, int relu, float* y, float* mean /*[c]*/, float* invstd /*[c]*/,
                         float* var_unbiased /*[c]*/, void* workspace, int64_t workspace_bytes, void* stream);
int dca_bn_train_backward(const float* dy, const float* x, const float* y /*needed if relu*/, const float* mean,
                          const float* invstd, const float* gamma, int64_t n, int64_t c, int relu, float* dx,
                          float* dskip /*or NULL*/, float* dgamma /*[c]*/, float* dbeta /*[c]*/, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Heuristic network, first layer: y = relu?( onehot(states_nnet, depth) . W1^T + b1 ) straight from the
 * uint8 network-input rows — utils/pytorch_models.py:49-60 with BatchNorm folded — as one MFMA kernel that never
 * materialises the one-hot matrix.  Weights arrive as `planes` bf16 planes whose sum is the fp32 weight matrix
 * (planes = 3: exact fp32 products => an fp32 GEMM on the bf16 MFMA pipes; 2 for fp16 weights; 1 for bf16), tiled as
 * [n_pad/64][planes][k_pad/8][64][8] (k_pad = dca_l1_kpad(state_dim, depth), zero padded; deepcubea_amd/utils/
 * pytorch_models.py:l1_weight_tiles builds it).  out: [m, n_pad] in out_dtype (DCA_DT_*), row stride n_pad; DCA_DT_F16_PLANES
 * writes the next layer's dca_f16x3_gemm operand directly ([m, n_pad] fp16 high halves, then [m, n_pad] low halves).
 * K is walked in LDS-sized chunks (cube3: one piece; the sliding puzzles, K up to 2401: 320 one-hot columns at a time).
 * Instantiated for cube3 (54, 6) and the sliding puzzles (9/16/25/36/49): dca_l1_supported(state_dim, depth) != 0.
 * ------------------------------------------------------------------------------------------------------------------ */
int dca_l1_supported(int state_dim, int depth);
int64_t dca_l1_kpad(int state_dim, int depth);
int dca_l1_onehot_gemm(const uint8_t* nnet_in /*[m, state_dim]*/, int64_t m, int state_dim, int depth, const void* w_tiles,
                       int planes, int64_t n_pad, const float* bias /*[n_pad]*/, int relu, void* out, int out_dtype,
                       int* overflow /*device flag, set to 1 if a DCA_DT_F16_PLANES value exceeds fp16; or NULL*/, void* stream);

/* The same layer in the NON-parity fp8 mode, on gfx950's f8f6f4 matrix pipe (csrc/dca_mlp8.hip): a one-hot row is exact in
 * OCP e4m3, so with the layer's weights as e4m3 bytes + one fp32 scale per output unit (what every other fp8 layer carries)
 *   out8[r, n] = e4m3(sat( relu?( (onehot(s_r) . w8[n, :]) * scale[n] + bias[n] ) ))
 * runs on v_mfma_f32_32x32x64_f8f6f4 — twice the rate of the bf16 pipe dca_l1_onehot_gemm(..., DCA_DT_E4M3) multiplies the same
 * exact 0 / 1 rows on.  The caller folds the activation scale of the output tensor into scale[] and bias[].
 * w_tiles: [n_pad/128][k_pad/16][128][16] e4m3 bytes, k_pad = dca_l1_kpad8(state_dim, depth) (K zero padded to a multiple of 64;
 * deepcubea_amd/utils/pytorch_models.py:l1_weight_tiles8 builds it); n_pad % 128 == 0; nnet_in and out8 16-byte aligned;
 * out8: [m, n_pad] bytes.  Instantiated where the 128-column weight tile fits LDS: dca_l1_supported8() != 0 (cube3,
 * puzzle8, puzzle15, puzzle24, lightsout7); other geometries keep the bf16-pipe kernel. */
int dca_l1_supported8(int state_dim, int depth);
int64_t dca_l1_kpad8(int state_dim, int depth);
int dca_l1_onehot_gemm8(const uint8_t* nnet_in /*[m, state_dim]*/, int64_t m, int state_dim, int depth, const void* w_tiles,
                        int64_t n_pad, const float* scale /*[n_pad]*/, const float* bias /*[n_pad]*/, int relu, void* out8,
                        void* stream);

/* The same layer as an EMBEDDING SUM on the vector pipes (csrc/dca_embed.hip): a one-hot row has one 1 per position, so
 *   out[r, n] = relu?( bias[n] + sum_pos w_t[pos * depth + s[r, pos]][n] )          (positions in ascending order, fp32 adds)
 * — state_dim gathered weights per output instead of state_dim * depth multiply-adds, in exact fp32 arithmetic with no operand
 * splitting.  It pays where depth is large (the sliding puzzles: depth = the tile count; puzzle48: 49 of 2401 columns are ones);
 * cube3 (depth 6) is faster on the matrix pipes (dca_l1_onehot_gemm).  w_t: the layer's weight matrix TRANSPOSED, fp32
 * [state_dim * depth][n_pad] (row = one-hot column); bias [n_pad]; n_pad % 64 == 0; nnet_in, w_t, out 16-byte aligned.
 * out_dtype: DCA_DT_F32 [m, n_pad], DCA_DT_BF16 [m, n_pad], or DCA_DT_F16_PLANES (dca_f16x3_gemm's operand: [m, n_pad] fp16
 * high halves, then [m, n_pad] low halves; *overflow set to 1 if a value exceeds fp16), or DCA_DT_E4M3 [m, n_pad] bytes,
 * saturating (the caller has folded the activation scale into w_t and bias).  State bytes must be < depth.
 * Instantiated for the geometries dca_l1_embed_supported() names (cube3, puzzle8/15/24/35/48, lightsout7). */
int dca_l1_embed_supported(int state_dim, int depth);
int dca_l1_embed(const uint8_t* nnet_in /*[m, state_dim]*/, int64_t m, int state_dim, int depth, const float* w_t, int64_t n_pad,
                 const float* bias /*[n_pad]*/, int relu, void* out, int out_dtype, int* overflow /*device flag or NULL*/,
                 void* stream);

/* The TRAINING step's layer 1 from the uint8 rows (csrc/dca_embed_train.hip): the reference's loss.backward()
 * (utils/nnet_utils.py:53-118) computes fc1's weight gradient of utils/pytorch_models.py:49-60 as the GEMM dy^T . onehot(s); with
 * one 1 per position that is a scatter, the gradient of the embedding sum above (whose fp32 output is the forward):
 *   dW[j, pos * depth + v] = sum over the rows r with s[r, pos] == v of dy[r, j]          db[j] = sum over all rows r of dy[r, j]
 * dW is WRITTEN (not accumulated into) in nn.Linear's own layout [n][K], K = state_dim * depth, row stride ldw >= K (elements
 * K..ldw of a row are not touched); a column no row selects comes out as +0.0.  nnet_in: uint8 [m, state_dim]; dy: fp32 [m, n],
 * row stride ld_dy >= n, 16-byte aligned, ld_dy % 4 == 0; n % 4 == 0; db: [n], or NULL to skip it.
 * Summation order (part of the contract: a value has the same bits on every launch, and a host loop reproduces them): the rows
 * are cut into consecutive slices of S = dca_l1_embed_wgrad_slice_rows(state_dim, depth) rows, the last one shorter — S depends
 * on the geometry alone, never on m or n (0 would mean: one slice); within a slice every element of dW and db is a sequential
 * fp32 sum over the rows in ascending order, starting from +0.0; the slices' sums are then added in ascending slice order, in
 * fp32, again from +0.0.  S today: 1024 for cube3 (54, 6), puzzle8 (9, 9), puzzle15 (16, 16) and lightsout7 (49, 6); 2048 for
 * puzzle24 (25, 25), puzzle35 (36, 36) and puzzle48 (49, 49) — read it from the accessor, these are the values the order rule has.
 * State bytes: the forward's contract is "< depth".  Here a position whose byte is >= depth contributes NOTHING to dW (a bad byte
 * would otherwise be a write to another position's rows); its row still counts in db.
 * workspace: dca_l1_embed_wgrad_workspace_bytes(m, state_dim, depth, n) bytes of device memory, 4-byte aligned (the slices'
 * partial tables; 0 bytes — NULL is fine — while m <= S).  m == 0 writes zeros.  DCA_E_BADARG, with a message and without a
 * launch, for: a geometry dca_l1_embed_supported() does not name, n % 4 != 0, m < 0, a NULL nnet_in / dy / dW, a misaligned dy
 * or ld_dy, ldw < K, ld_dy < n, a workspace that is missing or too small (the two accessors return DCA_E_BADARG likewise). */
int64_t dca_l1_embed_wgrad_slice_rows(int state_dim, int depth);
int64_t dca_l1_embed_wgrad_workspace_bytes(int64_t m, int state_dim, int depth, int64_t n);
int dca_l1_embed_wgrad(const uint8_t* nnet_in /*[m, state_dim]*/, int64_t m, int state_dim, int depth, const float* dy, int64_t ld_dy,
                       int64_t n, float* dW, int64_t ldw, float* db /*[n] or NULL*/, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* Glue in front of the fp32-accurate "f16x3" dense layers (csrc/dca_mlp.hip): v = relu?(y*alpha*col_scale + bias (+ skip)) over a
 * row-major fp32 GEMM output y [m, n] (layer 1 on materialised one-hot rows); writes dca_f16x3_gemm's operand `planes` — [m, n]
 * fp16 high halves vh = f16(v), then [m, n] low halves vl = f16(v - vh) — and / or, if x_out != NULL, v itself.  n % 4 == 0. */
int dca_act_split(const float* y, const float* bias /*[n] or NULL*/, const float* skip /*[m,n] or NULL*/,
                  const float* col_scale /*[n] or NULL: per-output-unit inverse weight scale*/, double alpha, int relu,
                  int64_t m, int64_t n, float* x_out /*[m,n] or NULL*/, void* planes /*[2][m][n] fp16 or NULL*/,
                  int* overflow /*device flag, set to 1 if some |v| > 60000 (not splittable into fp16); or NULL*/,
                  void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Heuristic network, dense layers: v = relu?( (x . W^T) * alpha * col_scale + bias (+ skip) ) — one layer
 * of utils/pytorch_models.py:57-86 with BatchNorm folded — as ONE hand-written MFMA kernel with fp32 accuracy on the f16
 * matrix pipes ("f16x3": x = xh + xl, w = wh + wl in fp16; x.w = xl.wh + xh.wl + xh.wh accumulated in fp32; csrc/dca_gemm.hip).
 * Operands are fp16 PLANES: a_h / a_l [m, lda] (high / low halves of the fp32 activations: what this kernel, dca_l1_onehot_gemm
 * (DCA_DT_F16_PLANES), dca_act_split and dca_split_planes emit), w_h / w_l [n, ldw] (rows = output units,
 * pre-scaled by the power of two 1 / col_scale[row]).  k % 64 == 0; lda, ldw % 8 == 0; 16-byte aligned bases.
 * Outputs (row stride ldo): out_h / out_l — the result's planes, i.e. the NEXT layer's operand — and / or x_out, the fp32
 * result (the next residual block's skip, or the input of the 1-wide output layer).  overflow: device flag set when a value
 * does not fit fp16 (|v| > 60000; the caller then redoes the batch with fp32 GEMMs), or NULL.
 * Any m >= 0, any n >= 1 (m == 0 returns 0 without a launch); lda, ldw >= k; ldo >= n and ldo % 4 == 0; out_h / out_l: both or
 * neither, 8-byte aligned; x_out / skip 16-byte aligned; at least one output.  a_h / a_l may start at any 16-byte aligned column
 * of wider matrices.  Only [0, m) x [0, n) of an output is written (row stride ldo): columns n..ldo and rows from m keep their bytes.
 * ------------------------------------------------------------------------------------------------------------------ */
int dca_f16x3_gemm(const void* a_h, const void* a_l, int64_t m, int k, int64_t lda, const void* w_h, const void* w_l, int n,
                   int64_t ldw, const float* col_scale /*[n] or NULL*/, double alpha, const float* bias /*[n] or NULL*/,
                   const float* skip /*[m, ldo] fp32 or NULL*/, int relu, void* out_h, void* out_l, float* x_out, int64_t ldo,
                   int* overflow, void* stream);

/* The same layer in the NON-parity 16-bit modes (`--nnet_dtype bf16 | fp16`; replaces the library GEMM + separate clamp pass of
 * utils/pytorch_models.py:57-86 as PyTorch runs it): out = relu?( a . w^T + bias (+ skip) ), operands and result in `dtype`
 * (DCA_DT_BF16 or DCA_DT_F16), fp32 accumulation on the 16-bit MFMA pipes, bias fp32, the residual `skip` [m, ldo] in
 * `dtype`, result rounded to nearest even — bias, residual add, ReLU and rounding ride in the epilogue (csrc/dca_gemm16.hip).
 * a [m, lda], w [n, ldw] (rows = output units); k % 64 == 0; lda, ldw % 8 == 0; ldo % 4 == 0; a / w 16-byte, out / skip
 * 8-byte aligned.  `out` may not alias `a` — a byte range [out, out + ((m - 1) ldo + n) elements) that meets a's is refused with
 * DCA_E_BADARG —; it may be `skip` itself (the in-place residual).  Any m >= 0, n >= 1; only [0, m) x [0, n) of `out` is
 * written.  out / skip that are 8- but not 16-byte aligned, or ldo % 8 != 0, are served by the general tail: same bits. */
int dca_gemm16(const void* a, int64_t m, int k, int64_t lda, const void* w, int n, int64_t ldw, int dtype,
               const float* bias /*[n] or NULL*/, const void* skip /*[m, ldo] or NULL*/, int relu, void* out, int64_t ldo,
               void* stream);

/* The same layer in the NON-parity fp8 mode (`--nnet_dtype fp8`; csrc/dca_gemm8.hip): OCP e4m3 operands a [m, lda] / w [n, ldw]
 * (bytes; k % 128 == 0, lda / ldw % 16 == 0), fp32 accumulation on v_mfma_f32_32x32x64_f8f6f4, and the whole tail in the epilogue:
 *   v = relu?( (a . w^T)[m,n] * scale[n] + bias[n] (+ skip[m,n]) )        scale[n] = activation scale x weight scale of unit n
 * leaving as bf16 (out16 [m, ldo16], the residual stream; may be `skip` itself) and / or quantised for the next layer:
 * out8 [m, ldo8] = e4m3(sat(v * out8_scale)).  skip is bf16 with out16's row stride.  Replaces utils/pytorch_models.py:57-86
 * (BatchNorm folded) as PyTorch runs it, at fp8 operand precision: never a parity mode.
 * a / w 16-byte aligned; out16 / skip 8-byte aligned, ldo16 >= n and % 4 == 0 (wanted whenever out16 or skip is given); out8
 * 4-byte aligned, ldo8 >= n and % 4 == 0, out8_scale > 0; at least one output.  An out16 or out8 whose bytes meet a's is refused
 * with DCA_E_BADARG.  Any m >= 0, n >= 1; only [0, m) x [0, n) of an output is written. */
int dca_gemm8(const void* a, int64_t m, int k, int64_t lda, const void* w, int n, int64_t ldw, const float* scale /*[n]*/,
              const float* bias /*[n] or NULL*/, const void* skip /*bf16 [m, ldo16] or NULL*/, int relu, void* out16 /*or NULL*/,
              int64_t ldo16, void* out8 /*or NULL*/, int64_t ldo8, double out8_scale, void* stream);
/* Block-scaled ("MX") form of the fp8 layer — what `--nnet_dtype fp8` runs: activations travel as e4m3 bytes PLUS one E8M0 scale
 * byte (value 2^(byte - 127)) per row and 64 consecutive elements, computed where the activation is produced (the largest
 * magnitude of the 64 values sets the power of two that brings them into e4m3's range) and applied by gfx950's scaled MFMA
 * (v_mfma_scale_f32_32x32x64_f8f6f4: both lane halves of a row pass the row's scale of the 64-deep step; the weights pass
 * 2^0 and keep their per-output-unit fp32 scales w_scale[n] for the epilogue).  No calibration, nothing frozen, no saturation:
 *   v = relu?( (sum_blocks 2^(sa - 127) * a8 . w8^T)[m,n] * w_scale[n] + bias[n] (+ skip[m,n]) )
 * a_scale [m, ld_asc] (k / 64 bytes per row; k % 256 == 0, k <= 8192); out8 / out8_scale [m, ld_osc] (n / 64 bytes per row,
 * n % 64 == 0) = the next layer's operand and its block scales, or both NULL; out16 / skip as in dca_gemm8.
 * a_scale 4-byte aligned, ld_asc >= k / 64 and % 4 == 0; ld_osc >= n / 64.  Refused with DCA_E_BADARG: one of out8 / out8_scale
 * without the other, an output whose bytes meet a's, out8_scale == a_scale.  Only [0, m) x [0, n) of out16 / out8 and
 * [0, m) x [0, n / 64) of out8_scale are written.
 * dca_l1_onehot_gemm_mx: layer 1 (one bf16 weight plane, dca_l1_onehot_gemm's tiles) leaving in the same form. */
int dca_gemm8_mx(const void* a, const void* a_scale, int64_t m, int k, int64_t lda, int64_t ld_asc, const void* w, int n,
                 int64_t ldw, const float* w_scale /*[n]*/, const float* bias /*[n] or NULL*/,
                 const void* skip /*bf16 [m, ldo16] or NULL*/, int relu, void* out16 /*or NULL*/, int64_t ldo16,
                 void* out8 /*or NULL*/, int64_t ldo8, void* out8_scale /*or NULL*/, int64_t ld_osc, void* stream);
int dca_l1_onehot_gemm_mx(const uint8_t* nnet_in /*[m, state_dim]*/, int64_t m, int state_dim, int depth, const void* w_tiles,
                          int64_t n_pad, const float* bias /*[n_pad]*/, int relu, void* out8 /*[m, n_pad] e4m3*/,
                          void* out_scale /*[m, ld_sc] E8M0*/, int64_t ld_sc, void* stream);
/* x [m, n] (row stride ld; DCA_DT_F32 or DCA_DT_BF16) -> e4m3(sat(x * scale)) bytes [m, ldo]: the entry into an fp8 layer for
 * activations that did not come out of an fp8 epilogue.  n % 4 == 0, ld % 4 == 0, ldo % 4 == 0, scale > 0; x 16-byte (fp32) or
 * 8-byte (bf16), out 4-byte aligned; only [0, m) x [0, n) of out is written. */
int dca_quant_e4m3(const void* x, int dtype, int64_t m, int64_t n, int64_t ld, double scale, void* out, int64_t ldo, void* stream);
/* fp32 [m, n] (row stride ld) -> its fp16 planes (row stride ldo); n % 4 == 0, ld % 4 == 0, ldo % 4 == 0, x 16-byte and the
 * planes 8-byte aligned; only [0, m) x [0, n) of a plane is written. */
int dca_split_planes(const float* x, int64_t m, int64_t n, int64_t ld, void* out_h, void* out_l, int64_t ldo,
                     int* overflow /*or NULL*/, void* stream);

/* Operands of the TRAINING step's dense layers (nn.Linear forward y = x . W^T and backward dx = dy . W of
 * utils/nnet_utils.py:53-118 through dca_f16x3_gemm; deepcubea_amd/_lib.py linear_train).  Nothing is prepared ahead here —
 * the weights change every step, gradients span many binades — so every operand is scaled by a power of two taken from its own
 * magnitude before it is split (exact), and the inverse scales return through the GEMM's col_scale:
 *   dca_absmax_bits          max |x| of an fp32 matrix as float bits, into a device word (zeroed here)
 *   dca_split_planes_scaled  x * 2^e -> fp16 planes, 2^e taking max|x| (amax_bits, from dca_absmax_bits) into [2^14, 2^15);
 *                            amax_bits NULL = unscaled; columns n..n_pad are written as zeros (the GEMM wants k % 64 == 0)
 *   dca_split_rows_scaled    per ROW of w [n, k]: the row's own 2^e, its planes (columns k..k_pad zero) and
 *                            col_scale[row] = 1 / (2^e * the other operand's scale, when other_amax_bits is given)
 * n, k, n_pad, k_pad % 4 == 0; 16-byte aligned inputs. */
int dca_absmax_bits(const float* x, int64_t m, int64_t n, int64_t ld, uint32_t* out_bits, void* stream);
int dca_split_planes_scaled(const float* x, int64_t m, int64_t n, int64_t ld, const uint32_t* amax_bits /*device or NULL*/,
                            void* out_h, void* out_l, int64_t ldo, int64_t n_pad, void* stream);
int dca_split_rows_scaled(const float* w, int64_t n, int64_t k, int64_t ld, void* out_h, void* out_l, int64_t ldo, int64_t k_pad,
                          float* col_scale /*[n]*/, const uint32_t* other_amax_bits /*device or NULL*/, void* stream);
/* dca_fill_inv_pow2: out[0..n) = 2^-e of the power-of-two scale dca_split_planes_scaled derives from amax_bits. */
int dca_fill_inv_pow2(float* out, int64_t n, const uint32_t* amax_bits, void* stream);

/* The NON-parity mode of the training step's forward and input-gradient GEMMs (`--train_gemm f16`; csrc/dca_gemm.hip): the
 * scaled HIGH fp16 planes alone — 11-bit operands, one product per K-step instead of three, fp32 accumulation on
 * v_mfma_f32_16x16x32_f16, fp32 output:
 *   x_out[r, c] = (alpha * col_scale[c]) * sum over q < k of a_h[r, q] * w_h[c, q] + bias[c]            r < m, c < n
 * a_h [m, lda] / w_h [n, ldw] fp16, rows = output units: plane 0 of dca_split_planes_scaled / dca_split_rows_scaled, or what
 * the two casts below write.  No low planes, no skip, no ReLU, no plane outputs.  Same tile, tile map and epilogue as
 * dca_f16x3_gemm; no split-K and no atomics: the same input gives the same bits on every launch.  Only x_out[0..m, 0..n) is
 * written (row stride ldo).  Argument rules as dca_f16x3_gemm: k >= 64 and k % 64 == 0; lda, ldw >= k and % 8 == 0; ldo >= n
 * and % 4 == 0; a_h, w_h, x_out 16-byte aligned; n >= 1; m >= 0 (m == 0: returns 0, writes nothing).  Anything else is refused
 * with DCA_E_BADARG before a launch.
 *   dca_cast_planes_scaled / dca_cast_rows_scaled: dca_split_planes_scaled / dca_split_rows_scaled without the low plane —
 *   the same argument rules, scale, zero padding and col_scale; out_h bit for bit their high plane; half the bytes written. */
int dca_f16_gemm(const void* a_h, int64_t m, int k, int64_t lda, const void* w_h, int n, int64_t ldw,
                 const float* col_scale /*[n] or NULL*/, double alpha, const float* bias /*[n] or NULL*/, float* x_out, int64_t ldo,
                 void* stream);
int dca_cast_planes_scaled(const float* x, int64_t m, int64_t n, int64_t ld, const uint32_t* amax_bits /*device or NULL*/,
                           void* out_h, int64_t ldo, int64_t n_pad, void* stream);
int dca_cast_rows_scaled(const float* w, int64_t n, int64_t k, int64_t ld, void* out_h, int64_t ldo, int64_t k_pad,
                         float* col_scale /*[n]*/, const uint32_t* other_amax_bits /*device or NULL*/, void* stream);

/* Weight gradient of a dense layer of the training step from the planes above (csrc/dca_wgrad.hip; `--wgrad f16x3 | f16`):
 *   dw[j, c] = 2^-(e_dy + e_x) * sum over rows r < m of dy[r, j] * x[r, c]            j < n, c < k, fp32 accumulation
 * Plane convention: dy_h / dy_l [m, ld_dy] and x_h / x_l [m, ld_x] fp16 as dca_split_planes_scaled writes them — vh = f16(v * 2^e),
 * vl = f16(v * 2^e - vh), row = batch index — with columns n..pad64(n) and k..pad64(k) ZERO (pad64 = next multiple of 64; the
 * kernel reads them).  amax_dy_bits / amax_x_bits: the device words the planes were scaled by (2^e as dca_split_planes_scaled
 * derives it); NULL = scale 1.
 * Arithmetic: products = 3: dyh.xh + dyh.xl + dyl.xh (no lo.lo term), fp32-accurate like dca_f16x3_gemm; products = 1: dyh.xh
 * alone — 11-bit operands, fp32 accumulation, a NON-parity speed mode (the low planes may be NULL).  v_mfma_f32_16x16x32_f16 on
 * row-major K-tiles read with ds_read_b64_tr_b16: nothing is transposed in memory.
 * Slice rule: the rows are cut into S = dca_wgrad_splits(m, n, k) slices of equal length (a multiple of 32, the last one ragged),
 * S a function of the three sizes alone.  S == 1: one kernel, no workspace.  S > 1: every slice's partial tile goes to the fp32
 * workspace [S][n][k] (dca_wgrad_workspace_bytes = S * n * k * 4; 0 when S == 1) and a second kernel adds the slices in ascending
 * slice order, then applies the power-of-two scale.  No atomics: the same input gives the same bits on every launch.
 * Only dw[0..n, 0..k) is written (row stride ld_dw >= k).  Refused with DCA_E_BADARG before any HIP call: products not 1 or 3;
 * n or k not a positive multiple of 4; m < 1; ld_dy < pad64(n) or ld_x < pad64(k); a plane stride not a multiple of 8; ld_dw < k;
 * NULL operands (products = 3: a NULL low plane) or planes off the 16-byte grid (dw, workspace, amax words: 4 bytes); a workspace
 * that is too small. */
int dca_wgrad_splits(int64_t m, int n, int k);
int64_t dca_wgrad_workspace_bytes(int64_t m, int n, int k);
int dca_wgrad_f16(const void* dy_h, const void* dy_l /*or NULL*/, int64_t ld_dy, const void* x_h, const void* x_l /*or NULL*/,
                  int64_t ld_x, int64_t m, int n, int k, const uint32_t* amax_dy_bits /*device or NULL*/,
                  const uint32_t* amax_x_bits /*device or NULL*/, int products, float* dw, int64_t ld_dw, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* Output layer of the cost-to-go network (utils/pytorch_models.py:83-86, fc_out: res_dim -> out_dim, out_dim = 1 for every
 * environment of the reference): out[m, n_out] = x[m, k] . w[n_out, k]^T + bias, float64 accumulation in a FIXED order (one wave
 * per row, lane-strided FMA chains, xor-butterfly fold, one rounding to fp32): a row's value does not depend on its position, on m or on the launch
 * — the library GEMV this replaces chose its kernel (and summation order) from m.  x: DCA_DT_F32 / F16 / BF16 rows (row
 * stride ldx elements, k % 4 == 0, ldx % 4 == 0); w, bias, out fp32; n_out <= 8.  DCA_DT_F64 rows (16-byte aligned): the float64
 * sum is rounded to fp32 once, after the bias.  dca_head_gemv64: the same sum over float64 rows, left in float64 (out [m, n_out]). */
int dca_head_gemv(const void* x, int x_dtype, int64_t m, int k, int64_t ldx, const float* w /*[n_out, k]*/,
                  const float* bias /*[n_out] or NULL*/, int n_out, float* out /*[m, n_out]*/, void* stream);
int dca_head_gemv64(const double* x, int64_t m, int k, int64_t ldx, const float* w /*[n_out, k]*/, const float* bias /*[n_out] or NULL*/,
                    int n_out, double* out /*[m, n_out]*/, void* stream);

/* The float64 heuristic mode (`--nnet_dtype fp64`; csrc/dca_gemm64.hip): utils/pytorch_models.py:49-86 (BatchNorm folded in
 * float64) evaluated in float64 from the fp32 weights, rounded once to fp32 by dca_head_gemv (DCA_DT_F64).
 * dca_gemm64: one dense layer, out[m, n] (row stride ldo) = relu?( a[m, k] . w[n, k]^T + bias[n] (+ skip[m, n]) ), float64
 * throughout, on v_mfma_f64_16x16x4_f64; every output element summed over k in ascending order by one lane (no split-K), so a
 * row's value does not depend on m or on its position.  k % 2 == 0, lda / ldw even, a and w 16-byte aligned; bias may be NULL;
 * skip has out's row stride and may be `out` itself (the residual form), never `a`.
 * dca_l1_embed64: layer 1 as an embedding sum in float64 (one gathered weight per position, as dca_l1_embed):
 *   out[r, j] = relu?( bias[j] + sum_pos w_t[pos * depth + s[r, pos]][j] )           (bias first, positions ascending)
 * w_t = W1^T float64 [state_dim * depth][n_pad] (n_pad % 8 == 0), bias [n_pad], out [m, n_pad].  Any geometry whose table fits
 * LDS in 8 columns (160 KB: puzzle48's 2401 rows fit, so every environment of the product).  State bytes must be < depth. */
int dca_gemm64(const double* a, int64_t m, int k, int64_t lda, const double* w, int n, int64_t ldw, const double* bias /*[n] or NULL*/,
               const double* skip /*[m, ldo] or NULL*/, int relu, double* out, int64_t ldo, void* stream);
int dca_l1_embed64(const uint8_t* nnet_in /*[m, state_dim]*/, int64_t m, int state_dim, int depth, const double* w_t, int64_t n_pad,
                   const double* bias /*[n_pad]*/, int relu, double* out /*[m, n_pad]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCA_H_ */
