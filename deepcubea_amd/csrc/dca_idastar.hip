// dca_idastar.hip — iterative-deepening A* on the pattern databases (include/dca.h "IDA*"): optimal solutions with no OPEN, no
// CLOSED and no node pool.  Memory is the tables plus a packed move stack per lane.
//
//   frame    ida_lane<D> is one depth-first search as a flat state machine over a domain D (the sliding puzzles of dim 3, 4, 5;
//            cube3).  One loop iteration handles one node: the lane makes the next child of its current node, evaluates h, and
//            either descends (f <= T), goes on to the next sibling, or — no sibling left — backtracks by undoing its last move
//            (moves invert with a ^ 1: no stack of states, only the move stack, kept in LDS).  The state lives in registers: the
//            puzzles' board packed 4 or 5 bits a position with the blank and one running table index per pattern, cube3's two
//            words of cubie locations.  The same function, compiled for the host, is the sequential search of
//            dca_idastar_host (include/dca_debug.h).
//   reflect  PzDomain<DIM, true>: the puzzles' search on the reflected look-up (include/dca.h) — a second running index per
//            pattern, that of the state's mirror image, in the other half of the lane's eight, and h the larger of the two sums.
//   sym      C3SymDomain: cube3's search on the symmetric look-ups (include/dca.h) — the same state and moves, h the largest byte
//            over a look-up list in global memory, left at the first value that already prunes the child (BOUNDED).
//   dual     C3DualDomain: the symmetric search with the dual look-ups (include/dca.h) — where the list at the state does not
//            prune the child, the lane inverts its two words in registers and reads the list again at the inverse state.
//   kernels  ida_puzzle_kernel<DIM, REFLECT>, and ONE ida_cube3_kernel<D> for C3Domain, C3SymDomain and C3DualDomain: a domain
//            names the kernel's argument (Arg), makes a lane's Ctx from the staged move tables and that argument (ctx()), and
//            carries the kernel's name as messages give it (kernel_name).
//   host     ida_search<D> is every search's host frame: the root's table bytes, the argument's device memory and a control
//            block where a search will run on the device, ida_drive's threshold loop around one "device iteration or host lane"
//            body — the host lane's Ctx through the same D::ctx — and the block handed back.  ida_puzzle, ida_cube3 and
//            ida_cube3_sym only prepare their family's state, reads and argument.
//   batch    ida_puzzle_batch: many puzzle roots on one pattern set, one launch of ida_puzzle_batch_kernel<DIM, REFLECT> per
//            round — the next threshold of every root still searching, each root on its own blocks with its own control block.
//            A root's thresholds go through the same IdaRun steps as ida_drive's one root, so its results are the single search's.
//            ida_cube3_batch: the same for cube3 roots on one pattern set and look-up mode, ida_cube3_batch_kernel<D>, each root
//            with a bound on its solution's length (include/dca.h "bounded batches") — many shallow roots, such as the windows
//            of a found solution.  ida_batch_rounds is both families' rounds.
//   work     item i of an iteration names a move prefix of P moves, the mixed-radix digits of i (first move = most significant
//            digit; cube3: radix 12; puzzles: 4 for the first move, then 3 — a digit picks among the moves that do not undo
//            the one before).  A lane replays the prefix from the root under the pruning rules and the f <= T test and drops the item
//            where the prefix is pruned; below the prefix it searches depth first and never backtracks above it.  Items are
//            handed out by one agent-scope counter; a lane whose item is finished takes the next one in the same loop, so a wave
//            lives until the list is empty.  No lane waits for another: no barrier after the LDS staging, no spin.
//   counts   every retained child whose h is evaluated counts once.  A prefix node that several items replay is counted by the
//            item whose remaining digits are all 0, so a completed iteration's count does not depend on which lane ran what.
//   ending   the first lane at the goal claims a word by compare-and-swap and writes its moves; a lane adds its count to the
//            launch's counter every DCA_IDASTAR_POLL_NODES nodes (sooner under a tight budget: ida_poll), stops when that
//            passes the budget and polls the stop word there.  Whoever stops the launch also sets the item counter's top bit,
//            which ends every other lane's item fetch.
//
// Rates are in profiles/idastar_probe.txt; the reflected search against the plain one in profiles/idastar_reflect_probe.txt,
// the symmetric one in profiles/idastar_sym_probe.txt, the dual one in profiles/idastar_dual_probe.txt.
#include <cstdio>
#include <mutex>
#include <type_traits>
#include <vector>

#include "dca_pdb_cube3.h"
#include "dca_pdb_puzzle.h"

namespace dca {

constexpr int kIdaThreads = 256;
constexpr int kIdaMaxBlocks = DCA_IDASTAR_MAX_LANES / kIdaThreads;
constexpr int kIdaBlocksPerCu = 8;
constexpr int kIdaPuzzlePatterns = 8;  // running indices a lane keeps in registers
constexpr uint32_t kIdaPoll = DCA_IDASTAR_POLL_NODES;
constexpr uint32_t kIdaMaxT = DCA_IDASTAR_MAX_MOVES;  // thresholds above it: unsolvable
constexpr uint32_t kIdaNoMove = 0xFEu;                // "no previous move": matches no rule (even, and its face is no face)
constexpr uint32_t kIdaStopItems = 0x80000000u;       // the item counter's top bit: every later fetch is past the list's end
constexpr uint32_t kIdaSolved = 1u, kIdaBudget = 2u;  // bits of IdaCtrl::stop

// One launch's control block (device memory, or host memory for the host search); all zero in front of every launch.
struct IdaCtrl {
    unsigned long long nodes;  // counted nodes of this launch
    uint32_t next_item;
    uint32_t stop;
    uint32_t claim;   // 0 -> 1 by the lane that writes the solution
    uint32_t best;    // 0xFFFFFFFF - (the smallest f above T seen), 0 = none: a max, so that zero is "nothing yet"
    uint32_t length;  // of the solution
    uint32_t pad;
    uint8_t moves[256];
};

#define DCA_IDA_INLINE __host__ __device__ inline __attribute__((always_inline))
#define DCA_IDA_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ------------------------------------------------------------------------------------------------------ sliding puzzles
struct PzMaps {  // tile -> (its weight N^(digit) in its pattern's index, its pattern; 0xFF: the tile is in no pattern)
    uint64_t w[32];
    uint32_t p[32];
};
struct PzMapsReflect : PzMaps {  // and tile t -> the same of phi(t), the pattern as its slot np + p(phi(t)) of State::idx
    uint64_t rw[32];
    uint32_t rp[32];
};

template <bool REFLECT>
using PzMapsOf = std::conditional_t<REFLECT, PzMapsReflect, PzMaps>;

template <int DIM, bool REFLECT>
struct PzArgs;  // the kernel argument, behind the domain: it holds the root

// REFLECT: the reflected look-up (include/dca.h): slots np .. 2 np - 1 of State::idx are the running indices of the state's
// mirror image in the main diagonal, and h is the larger of the two sums.  Without it nothing below differs from the plain search.
template <int DIM, bool REFLECT = false>
struct PzDomain {
    using Arg = PzArgs<DIM, REFLECT>;
    static constexpr const char* kernel_name = "ida_puzzle_kernel";
    static constexpr int N = DIM * DIM, NM = 4, RADIX = 3, MOVE_BITS = 2, MAX_PREFIX = 15, STACK_WORDS = 16;
    static constexpr int BITS = N <= 16 ? 4 : 5;
    static constexpr bool BOUNDED = false;  // h(s, c): the whole value, whatever the threshold
    using Board = std::conditional_t<(N * BITS <= 64), uint64_t, unsigned __int128>;
    struct State {
        Board board;                        // position i holds tile (board >> BITS * i) & MASK
        uint32_t blank;                     // the blank's position
        uint64_t idx[kIdaPuzzlePatterns];  // per pattern: its table index without the blank digit
    };
    struct Ctx {
        const uint64_t* tile_w;
        const uint32_t* tile_p;
        const uint8_t* table[kIdaPuzzlePatterns];
        int np;
        const uint64_t* rtile_w;  // REFLECT only
        const uint32_t* rtile_p;
    };
    // what a lane reads: the tile maps where they stand (the kernel's copy in LDS, the host's own) and the argument's tables
    static DCA_IDA_INLINE Ctx ctx(const PzMapsOf<REFLECT>& maps, const Arg& a) {
        Ctx c;
        c.tile_w = maps.w;
        c.tile_p = maps.p;
        if constexpr (REFLECT) {
            c.rtile_w = maps.rw;
            c.rtile_p = maps.rp;
        }
#pragma unroll
        for (int q = 0; q < kIdaPuzzlePatterns; q++) c.table[q] = a.table[q];
        c.np = a.np;
        return c;
    }
    static int device_arg(Arg&) { return 0; }  // nothing of the argument is device memory of the search's own
    static constexpr Board MASK = (1u << BITS) - 1u;
    static constexpr Board goal_board() {
        Board b = 0;
        for (int i = 0; i < N; i++) b |= (Board)((i + 1) % N) << (BITS * i);
        return b;
    }

    // A prefix digit's move: the first digit is the move itself, a later one counts the moves other than the undo of m.
    static DCA_IDA_INLINE uint32_t digit_move(uint32_t d, uint32_t m) { return m == kIdaNoMove ? d : d + (d >= (m ^ 1u) ? 1u : 0u); }
    // Is a prefix depth p (that many items) worth it after an iteration of `prev` nodes?  A board has about 2.13 children a
    // node, so few of the items survive their replay and only a deep prefix feeds the chip; a dropped item costs a counter
    // add and the nodes up to its first illegal or pruned move, all lanes busy, and this iteration is several times `prev`.
    static bool worth(int64_t items, int, int64_t prev) { return items <= 8 * prev; }
    // the rules: no no-op move, no undoing of the previous move
    static DCA_IDA_INLINE bool legal(const State& s, uint32_t a, uint32_t m, uint32_t) {
        return a != (m ^ 1u) && (uint32_t)npuzzle_swap(DIM, (int)s.blank, (int)a) != s.blank;
    }
    // the blank trades places with the tile t at nb: t's digit goes nb -> blank in its pattern's index, the blank digit is added
    // at the gather.  (A no-op move — only ever asked for as a legal one — would leave the state as it is.)
    static DCA_IDA_INLINE State apply(const State& s, uint32_t a, const Ctx& c) {
        const uint32_t nb = (uint32_t)npuzzle_swap(DIM, (int)s.blank, (int)a);
        const uint32_t t = (uint32_t)((s.board >> (BITS * nb)) & MASK);
        State r;
        r.board = (s.board & ~(MASK << (BITS * nb))) | ((Board)t << (BITS * s.blank));
        r.blank = nb;
        const uint64_t w = c.tile_w[t];  // t < 2^BITS <= 32
        const uint32_t p = c.tile_p[t];
        const uint64_t delta = w * (uint64_t)s.blank - w * (uint64_t)nb;  // modulo 2^64: the sum is the exact index
        if constexpr (REFLECT) {
            // in the mirror image tile phi(t) goes refl(nb) -> refl(blank); p < np <= rp, so a slot takes one of the two deltas
            const uint64_t rw = c.rtile_w[t];
            const uint32_t rp = c.rtile_p[t];
            const uint64_t rdelta = rw * (uint64_t)pdb_refl<DIM>(s.blank) - rw * (uint64_t)pdb_refl<DIM>(nb);
#pragma unroll
            for (int q = 0; q < kIdaPuzzlePatterns; q++)
                r.idx[q] = s.idx[q] + (p == (uint32_t)q ? delta : 0ull) + (rp == (uint32_t)q ? rdelta : 0ull);
            return r;
        }
#pragma unroll
        for (int q = 0; q < kIdaPuzzlePatterns; q++) r.idx[q] = s.idx[q] + (p == (uint32_t)q ? delta : 0ull);
        return r;
    }
    static DCA_IDA_INLINE uint32_t h(const State& s, const Ctx& c) {
        if constexpr (REFLECT) {
            // slot np + q reads table q again (c.table[np + q] = c.table[q]): every slot is a constant register, and the 2 np
            // gathers are independent, all in flight before the first is summed
            const uint32_t rblank = pdb_refl<DIM>(s.blank);
            uint32_t v[kIdaPuzzlePatterns];
#pragma unroll
            for (int q = 0; q < kIdaPuzzlePatterns; q++) {
                v[q] = 0;
                if (q < 2 * c.np) v[q] = c.table[q][s.idx[q] + (q < c.np ? s.blank : rblank)];
            }
            uint32_t sum = 0, rsum = 0;
#pragma unroll
            for (int q = 0; q < kIdaPuzzlePatterns; q++) {
                sum += q < c.np ? v[q] : 0u;
                rsum += q < c.np ? 0u : v[q];
            }
            return sum > rsum ? sum : rsum;
        }
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < kIdaPuzzlePatterns; q++)
            if (q < c.np) sum += c.table[q][s.idx[q] + s.blank];  // every digit < N: inside the table
        return sum;
    }
    static DCA_IDA_INLINE bool goal(const State& s) { return s.board == goal_board(); }
};

// ---------------------------------------------------------------------------------------------------------------- cube3
struct C3Domain {
    static constexpr int NM = 12, RADIX = 12, MOVE_BITS = 4, MAX_PREFIX = 6, STACK_WORDS = 32;
    static constexpr bool BOUNDED = false;
    struct State {
        uint64_t corner, edge;  // c3_row_locs: 5 bits a cubie
    };
    struct Ctx {
        const uint8_t* mv;  // [2][12][24]: kind, move, location -> location
        const C3Set* set;
    };
    // Every cube3 domain: Arg, what ida_cube3_kernel<D> is handed; ctx(), what a lane reads, from the move tables where they
    // stand (LDS, or the host's words) and that argument; device_arg(), whatever of the argument needs a device copy.
    using Arg = C3Set;
    static constexpr const char* kernel_name = "ida_cube3_kernel";
    static DCA_IDA_INLINE Ctx ctx(const uint8_t* mv, const Arg& a) {
        Ctx c;
        c.mv = mv;
        c.set = &a;
        return c;
    }
    static int device_arg(Arg&) { return 0; }
    static constexpr uint64_t home(int n, int o) {
        uint64_t w = 0;
        for (int q = 0; q < n; q++) w |= (uint64_t)(q * o) << (5 * q);
        return w;
    }

    static DCA_IDA_INLINE uint32_t digit_move(uint32_t d, uint32_t) { return d; }
    // Is a prefix depth p worth it after an iteration of `prev` nodes?  Replaying every item's prefix (at most p nodes an
    // item) then costs less than half of the previous, 13 times smaller, iteration.
    static bool worth(int64_t items, int p, int64_t prev) { return items * p <= prev / 2; }
    // a = 2 face + dir: no undo; a half turn with the even action only; no third turn of a kind; opposite faces ascending
    static DCA_IDA_INLINE bool legal(const State&, uint32_t a, uint32_t m, uint32_t mp) {
        const uint32_t fa = a >> 1, fm = m >> 1;
        return !(a == (m ^ 1u) || (a == m && (a & 1u)) || (a == m && m == mp) || (fa == (fm ^ 1u) && fa < fm));
    }
    static DCA_IDA_INLINE State apply(const State& s, uint32_t a, const Ctx& c) {
        State r{0ull, 0ull};
        const uint8_t* mc = c.mv + a * kC3Locs;
        const uint8_t* me = c.mv + (12 + a) * kC3Locs;
#pragma unroll
        for (int q = 0; q < 8; q++) r.corner |= (uint64_t)mc[(s.corner >> (5 * q)) & 31u] << (5 * q);  // locations stay < 24
#pragma unroll
        for (int q = 0; q < 12; q++) r.edge |= (uint64_t)me[(s.edge >> (5 * q)) & 31u] << (5 * q);
        return r;
    }
    static DCA_IDA_INLINE uint32_t h(const State& s, const Ctx& c) {
        const C3Set& set = *c.set;
        uint32_t best = 0;
        for (int p0 = 0; p0 < set.np; p0 += 4) {  // four independent gathers in flight
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                v[q] = 0;
                const int pi = p0 + q;
                if (pi < set.np) {
                    const uint64_t idx = set.kind[pi] == DCA_CUBE3_CORNERS ? c3_index<DCA_CUBE3_CORNERS>(s.corner, set.pat[pi], set.k[pi])
                                                                           : c3_index<DCA_CUBE3_EDGES>(s.edge, set.pat[pi], set.k[pi]);
                    v[q] = set.table[pi][idx];
                }
            }
            const uint32_t x = v[0] > v[1] ? v[0] : v[1], y = v[2] > v[3] ? v[2] : v[3];
            best = best > x ? best : x;
            best = best > y ? best : y;
        }
        return best;
    }
    // every cubie at its home location (h = 0 is not the goal: a corners-only set is 0 on unsolved states)
    static DCA_IDA_INLINE bool goal(const State& s) { return s.corner == home(8, 3) && s.edge == home(12, 2); }
};

// cube3 on the symmetric look-ups (include/dca.h "Symmetric look-ups"): the same state, moves, rules and goal; h is the largest
// byte over the look-up list.  The list and its location maps stay in global memory: LDS — what bounds this kernel's occupancy —
// holds what the plain kernel's does.  A trip of four look-ups reads its four heads by scalar loads (the trip's number is
// wave-uniform), issues its 32 per-lane map reads together, ranks, and issues its four gathers together (c3_sym_gather4;
// checked in the generated code, profiles/cube3_sym_isa.txt).
struct C3SymDomain : C3Domain {
    static constexpr bool BOUNDED = true;  // h(s, c, slack) may stop at the first value above slack
    struct Ctx : C3Domain::Ctx {
        const C3SymList* list;
        int n;
    };
    using Arg = C3SymSet;
    static constexpr const char* kernel_name = "ida_cube3_sym_kernel";
    static DCA_IDA_INLINE Ctx ctx(const uint8_t* mv, const Arg& a) {
        Ctx c;
        c.mv = mv;
        c.set = nullptr;
        c.list = a.list;
        c.n = a.n;
        return c;
    }
    static int device_arg(Arg& a) { return c3_sym_device_list(*a.list, a.list); }
    // The largest byte over the list, or — the early exit — over its first look-ups once that is above `slack` = T - g - 1:
    // f > T either way, so the same children are pruned as under the full maximum; only the f a pruned child records for the
    // next threshold may be smaller than its exact f (include/dca.h: the thresholds of the exact search still all occur).
    static DCA_IDA_INLINE uint32_t h(const State& s, const Ctx& c, uint32_t slack) {
        uint32_t best = 0;
        for (int p0 = 0; p0 < c.n; p0 += 4) {  // four independent gathers in flight
            const uint32_t v = c3_sym_gather4(c.list, p0, s.corner, s.edge);
            best = best > v ? best : v;
            if (best > slack) break;
        }
        return best;
    }
};

// cube3 on the dual look-ups (include/dca.h "Dual look-ups"): the symmetric search's state, moves, rules, goal and list; h is
// the larger of the list's value at the state and at the inverse state.  The inverse is not kept in the lane's state — apply,
// the undo and the stack are the plain search's — but made from the child's two words where it is needed: only a child that
// the first pass does not prune pays for it (registers only, the or-only form: the root's slots are checked to be distinct).
// Admissible, NOT consistent: h of a child may be more than one below its parent's.  IDA* needs admissibility alone.
struct C3DualDomain : C3SymDomain {
    struct Ctx : C3SymDomain::Ctx {
        C3DualPass dual;
    };
    using Arg = C3DualSet;
    static constexpr const char* kernel_name = "ida_cube3_dual_kernel";
    static DCA_IDA_INLINE Ctx ctx(const uint8_t* mv, const Arg& a) {
        Ctx c;
        c.mv = mv;
        c.set = nullptr;
        c.list = a.list;
        c.n = a.n;
        c.dual = a.dual;
        return c;
    }
    static DCA_IDA_INLINE uint32_t h(const State& s, const Ctx& c, uint32_t slack) {
        const uint32_t best = C3SymDomain::h(s, c, slack);
        if (best > slack) return best;
        const uint64_t corner = (c.dual.kinds & 1) ? c3_inverse_locs<DCA_CUBE3_CORNERS, false>(s.corner) : 0ull;
        const uint64_t edge = (c.dual.kinds & 2) ? c3_inverse_locs<DCA_CUBE3_EDGES, false>(s.edge) : 0ull;
        return c3_dual_value(c.list, c.n, c.dual.lead, corner, edge, best, slack);
    }
};

// ------------------------------------------------------------------------------------------------------------ the frame
// One lane's share of one iteration (threshold T, prefix depth P, n_items = NM * RADIX^(P-1) < 2^31 work items).  stk: the lane's move
// stack, word w at stk[w * stride].  budget: the nodes this launch may still count; poll: the nodes between a lane's flushes.
template <typename D>
DCA_IDA_INLINE void ida_lane(const typename D::Ctx& c, const typename D::State& root, IdaCtrl* ctrl, uint32_t* stk, uint32_t stride,
                             uint32_t T, uint32_t P, uint32_t n_items, unsigned long long budget, uint32_t poll) {
    constexpr uint32_t PER = 32u / D::MOVE_BITS, MM = (1u << D::MOVE_BITS) - 1u, NM = D::NM;
    typename D::State s = root;
    uint32_t g = 0, item = 0, cursor = 0, m1 = kIdaNoMove, m2 = kIdaNoMove, since = 0, best = 0;
    bool have = false;
    const auto stack_get = [&](uint32_t d) { return (stk[(d / PER) * stride] >> ((d % PER) * D::MOVE_BITS)) & MM; };
    for (;;) {
        if (!have) {  // the next item, from the root
            item = __hip_atomic_fetch_add(&ctrl->next_item, 1u, DCA_IDA_RLX);
            if (item >= n_items) break;
            s = root;
            g = 0;
            cursor = 0;
            m1 = m2 = kIdaNoMove;
            have = true;
        }
        const bool replay = g < P;
        uint32_t a, below = 1;  // below = RADIX^(digits after this one)
        if (replay) {
            for (uint32_t d = g + 1; d < P; d++) below *= (uint32_t)D::RADIX;
            const uint32_t q = item / below;  // (the first digit's radix is NM: no digit above it)
            a = D::digit_move(g == 0u ? q : q % (uint32_t)D::RADIX, m1);
            if (!D::legal(s, a, m1, m2)) {
                have = false;
                continue;
            }
        } else {
            while (cursor < NM && !D::legal(s, cursor, m1, m2)) cursor++;
            if (cursor >= NM) {
                if (g == P) {  // the item's subtree is exhausted
                    have = false;
                    continue;
                }
                s = D::apply(s, m1 ^ 1u, c);  // backtrack: undo the last move, go on with its next sibling
                cursor = m1 + 1u;
                g--;
                m1 = m2;
                m2 = g >= 2u ? stack_get(g - 2u) : kIdaNoMove;
                continue;
            }
            a = cursor;
        }
        const typename D::State ch = D::apply(s, a, c);
        uint32_t f;
        if constexpr (D::BOUNDED)  // a bounded family is told how much room is left below T
            f = g + 1u + D::h(ch, c, T > g ? T - g - 1u : 0u);
        else
            f = g + 1u + D::h(ch, c);
        since += (!replay || item % below == 0u) ? 1u : 0u;  // a replayed node: counted by the item whose later digits are 0
        if (f <= T) {
            uint32_t* word = stk + (g / PER) * stride;
            const uint32_t sh = (g % PER) * D::MOVE_BITS;
            *word = (*word & ~(MM << sh)) | (a << sh);
            if (D::goal(ch)) {
                uint32_t free_word = 0u;  // the first claim writes; the host reads after the launch
                if (__hip_atomic_compare_exchange_strong(&ctrl->claim, &free_word, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT)) {
                    for (uint32_t d = 0; d <= g; d++) ctrl->moves[d] = (uint8_t)stack_get(d);
                    ctrl->length = g + 1u;
                }
                __hip_atomic_fetch_or(&ctrl->stop, kIdaSolved, DCA_IDA_RLX);
                __hip_atomic_fetch_or(&ctrl->next_item, kIdaStopItems, DCA_IDA_RLX);
                break;
            }
            s = ch;
            m2 = m1;
            m1 = a;
            g++;
            cursor = 0;
        } else {
            const uint32_t inv = 0xFFFFFFFFu - f;
            best = best > inv ? best : inv;
            if (replay)
                have = false;
            else
                cursor = a + 1u;
        }
        if (since >= poll) {
            const unsigned long long before = __hip_atomic_fetch_add(&ctrl->nodes, (unsigned long long)since, DCA_IDA_RLX);
            const bool over = before + since > budget;
            since = 0;
            if (over) {
                __hip_atomic_fetch_or(&ctrl->stop, kIdaBudget, DCA_IDA_RLX);
                __hip_atomic_fetch_or(&ctrl->next_item, kIdaStopItems, DCA_IDA_RLX);
                break;
            }
            if (__hip_atomic_load(&ctrl->stop, DCA_IDA_RLX) != 0u) break;
        }
    }
    if (since != 0u) __hip_atomic_fetch_add(&ctrl->nodes, (unsigned long long)since, DCA_IDA_RLX);
    if (best != 0u) __hip_atomic_fetch_max(&ctrl->best, best, DCA_IDA_RLX);
}

// -------------------------------------------------------------------------------------------------------------- kernels
template <int DIM, bool REFLECT>
struct PzArgs {
    typename PzDomain<DIM, REFLECT>::State root;
    const uint8_t* table[kIdaPuzzlePatterns];
    int np;
};

template <int DIM, bool REFLECT = false>
__global__ __launch_bounds__(kIdaThreads) void ida_puzzle_kernel(PzArgs<DIM, REFLECT> args, PzMapsOf<REFLECT> maps, IdaCtrl* ctrl, uint32_t T,
                                                                 uint32_t P, uint32_t n_items, unsigned long long budget, uint32_t poll) {
    using D = PzDomain<DIM, REFLECT>;
    __shared__ uint64_t tile_w[32];
    __shared__ uint32_t tile_p[32];
    __shared__ uint32_t stk[D::STACK_WORDS * kIdaThreads];
    if (threadIdx.x == 0) {  // (constant indices into the kernel argument: scalar loads, no private copy of the struct)
#pragma unroll
        for (int t = 0; t < 32; t++) {
            tile_w[t] = maps.w[t];
            tile_p[t] = maps.p[t];
        }
    }
    // (The context is filled here, not by D::ctx: staging the maps as one PzMaps in LDS for it moved the scalar loads and
    // renumbered the scalar registers of all six kernels, outside the machine-code rule.)
    typename D::Ctx c;
    if constexpr (REFLECT) {  // the second pair of tile maps, staged like the first
        __shared__ uint64_t rtile_w[32];
        __shared__ uint32_t rtile_p[32];
        if (threadIdx.x == 0) {
#pragma unroll
            for (int t = 0; t < 32; t++) {
                rtile_w[t] = maps.rw[t];
                rtile_p[t] = maps.rp[t];
            }
        }
        c.rtile_w = rtile_w;
        c.rtile_p = rtile_p;
    }
    __syncthreads();
    c.tile_w = tile_w;
    c.tile_p = tile_p;
#pragma unroll
    for (int q = 0; q < kIdaPuzzlePatterns; q++) c.table[q] = args.table[q];
    c.np = args.np;
    ida_lane<D>(c, args.root, ctrl, stk + threadIdx.x, kIdaThreads, T, P, n_items, budget, poll);
}

// A root of a batch as one round's launch reads it (device memory, uploaded in front of every round): the root, what
// ida_puzzle_kernel takes as launch parameters, and the first of the root's blocks in the round's grid.
template <int DIM, bool REFLECT>
struct PzBatchRoot {
    typename PzDomain<DIM, REFLECT>::State root;
    unsigned long long budget;
    uint32_t T, P, n_items, poll;
    uint32_t first_block;  // ascending over the round's roots, 0 for the first: root j owns first_block[j] .. first_block[j + 1] - 1
    uint32_t pad;
};

template <int DIM, bool REFLECT>
struct PzBatchArgs {
    const PzBatchRoot<DIM, REFLECT>* roots;  // [n_roots]
    uint32_t n_roots;                        // >= 1; the grid is the sum of the roots' blocks
    const uint8_t* table[kIdaPuzzlePatterns];
    int np;
};

// One round of a batch: the next threshold of every root still searching, root j on its own blocks with its own control
// block ctrl[j] — the pattern set and the tile maps are the batch's, staged as ida_puzzle_kernel stages them.  A block finds its
// root by a binary search of blockIdx.x in the descriptors' first blocks: kernel argument, block index and read-only memory
// only, so the search, the descriptor and the root sit in scalar registers (profiles/idastar_batch_isa.txt).
// The grid may be larger than what is resident, and then only queues: after the LDS staging no lane waits for any other lane
// or block — no barrier, no spin (ida_lane, "work") — so a block that starts late finds its root's item counter where the
// earlier ones left it, takes what is left or nothing, and ends.  A root that stops (solved, out of budget) closes only its own
// item counter, in its own control block; the other roots' blocks never read it.
// (The staging is written out again, not shared with ida_puzzle_kernel: as one inline function of both it moved that kernel's
// scalar loads in front, parked scalars in a VGPR's lanes and took the reflected kernels from 6 and 5 waves a SIMD to 4.)
template <int DIM, bool REFLECT = false>
__global__ __launch_bounds__(kIdaThreads) void ida_puzzle_batch_kernel(PzBatchArgs<DIM, REFLECT> args, PzMapsOf<REFLECT> maps, IdaCtrl* ctrl) {
    using D = PzDomain<DIM, REFLECT>;
    __shared__ uint64_t tile_w[32];
    __shared__ uint32_t tile_p[32];
    __shared__ uint32_t stk[D::STACK_WORDS * kIdaThreads];
    const PzBatchRoot<DIM, REFLECT>* __restrict__ roots = args.roots;
    uint32_t lo = 0, hi = args.n_roots;  // the last root whose first block is <= blockIdx.x (the first root's is 0)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (roots[mid].first_block <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const typename D::State root = roots[lo].root;  // read in front of every store: scalar loads, as the kernel argument's are
    const unsigned long long budget = roots[lo].budget;
    const uint32_t T = roots[lo].T, P = roots[lo].P, n_items = roots[lo].n_items, poll = roots[lo].poll;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int t = 0; t < 32; t++) {
            tile_w[t] = maps.w[t];
            tile_p[t] = maps.p[t];
        }
    }
    typename D::Ctx c;
    if constexpr (REFLECT) {
        __shared__ uint64_t rtile_w[32];
        __shared__ uint32_t rtile_p[32];
        if (threadIdx.x == 0) {
#pragma unroll
            for (int t = 0; t < 32; t++) {
                rtile_w[t] = maps.rw[t];
                rtile_p[t] = maps.rp[t];
            }
        }
        c.rtile_w = rtile_w;
        c.rtile_p = rtile_p;
    }
    __syncthreads();
    c.tile_w = tile_w;
    c.tile_p = tile_p;
#pragma unroll
    for (int q = 0; q < kIdaPuzzlePatterns; q++) c.table[q] = args.table[q];
    c.np = args.np;
    ida_lane<D>(c, root, ctrl + lo, stk + threadIdx.x, kIdaThreads, T, P, n_items, budget, poll);
}

struct C3IdaMoves {
    uint32_t w[2 * 12 * kC3Locs / 4];  // both kinds' location-move tables as words
};

// the plain, the symmetric and the dual search: what differs is the domain's argument and the context made from it
template <typename D>
__global__ __launch_bounds__(kIdaThreads) void ida_cube3_kernel(C3Domain::State root, typename D::Arg set, C3IdaMoves mt, IdaCtrl* ctrl, uint32_t T,
                                                                uint32_t P, uint32_t n_items, unsigned long long budget, uint32_t poll) {
    __shared__ uint32_t mvw[2 * 12 * kC3Locs / 4];
    __shared__ uint32_t stk[C3Domain::STACK_WORDS * kIdaThreads];
    if (threadIdx.x == 0) {  // (constant indices into the kernel argument: scalar loads, no private copy of the struct)
#pragma unroll
        for (int q = 0; q < 2 * 12 * kC3Locs / 4; q++) mvw[q] = mt.w[q];
    }
    __syncthreads();
    ida_lane<D>(D::ctx((const uint8_t*)mvw, set), root, ctrl, stk + threadIdx.x, kIdaThreads, T, P, n_items, budget, poll);
}

// A cube3 root of a batch as one round's launch reads it: PzBatchRoot's fields around the two location words.
struct C3BatchRoot {
    C3Domain::State root;
    unsigned long long budget;
    uint32_t T, P, n_items, poll;
    uint32_t first_block;  // ascending over the round's roots, 0 for the first
    uint32_t pad;
};

// One round of a cube3 batch, for the plain, the symmetric and the dual search: ida_puzzle_batch_kernel's scheme (the scalar
// binary search for the block's root, the root's own control block ctrl[j], a grid that may only queue) around
// ida_cube3_kernel<D>'s staging — the move tables once per block — and the unchanged ida_lane.  After the staging's barrier
// no lane waits for another lane or block.
template <typename D>
__global__ __launch_bounds__(kIdaThreads) void ida_cube3_batch_kernel(const C3BatchRoot* __restrict__ roots, uint32_t n_roots, typename D::Arg set,
                                                                      C3IdaMoves mt, IdaCtrl* ctrl) {
    __shared__ uint32_t mvw[2 * 12 * kC3Locs / 4];
    __shared__ uint32_t stk[C3Domain::STACK_WORDS * kIdaThreads];
    uint32_t lo = 0, hi = n_roots;  // the last root whose first block is <= blockIdx.x (the first root's is 0)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (roots[mid].first_block <= blockIdx.x)
            lo = mid;
        else
            hi = mid;
    }
    const C3Domain::State root = roots[lo].root;  // read in front of every store: scalar loads, as the kernel argument's are
    const unsigned long long budget = roots[lo].budget;
    const uint32_t T = roots[lo].T, P = roots[lo].P, n_items = roots[lo].n_items, poll = roots[lo].poll;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 2 * 12 * kC3Locs / 4; q++) mvw[q] = mt.w[q];
    }
    __syncthreads();
    ida_lane<D>(D::ctx((const uint8_t*)mvw, set), root, ctrl + lo, stk + threadIdx.x, kIdaThreads, T, P, n_items, budget, poll);
}

// ----------------------------------------------------------------------------------------------------------- host side
struct IdaOut {
    int* status;
    int* length;
    uint8_t* moves;
    int moves_cap;
    int* num_thresholds;
    int* thresholds;
    int64_t* nodes_per_threshold;
    int thresholds_cap;
    int64_t* total_nodes;
};

static int g_ida_forced_prefix = -1;  // dca_idastar_set_prefix

template <typename D>
static uint32_t ida_items(uint32_t P) {
    uint32_t n = P == 0u ? 1u : (uint32_t)D::NM;
    for (uint32_t d = 1; d < P; d++) n *= (uint32_t)D::RADIX;
    return n;
}

// The prefix depth of an iteration from the node count of the one before: the deepest P the family finds worth its items
// (D::worth); 0 — one item, one lane — for the first iterations.
template <typename D>
static uint32_t ida_prefix(int64_t prev_nodes) {
    if (g_ida_forced_prefix >= 0) return (uint32_t)(g_ida_forced_prefix < D::MAX_PREFIX ? g_ida_forced_prefix : D::MAX_PREFIX);
    uint32_t p = 0;
    while (p < (uint32_t)D::MAX_PREFIX && D::worth((int64_t)ida_items<D>(p + 1u), (int)p + 1, prev_nodes)) p++;
    return p;
}

// The nodes between a lane's flushes: DCA_IDASTAR_POLL_NODES, or less where the budget left is small against the lanes in
// flight — budget / (2 lanes), so that what the lanes hold unflushed stays under half of the budget (or one node a lane).
static uint32_t ida_poll(unsigned long long budget, int lanes) {
    const unsigned long long p = budget / (2ull * (unsigned long long)lanes);
    return (uint32_t)(p < 1 ? 1 : p < kIdaPoll ? p : kIdaPoll);
}

// One root's threshold loop as a state: what ida_drive keeps for its one root, and the batch driver per root.
struct IdaRun {
    IdaOut out;
    int64_t max_nodes, total, prev;  // prev: the count of the threshold before (0 in front of the first), what the prefix rule reads
    uint32_t T;                      // the next threshold
    uint32_t bound;                  // no threshold above it runs: kIdaMaxT, or the caller's bound on the solution's length
    int it;                          // thresholds run
    bool active;                     // a next threshold is to run

    // The root's outputs in front of any threshold; the search is over at once for a dead root and for the goal.
    void begin(uint32_t h_root, bool root_dead, bool root_goal, int64_t nodes, const IdaOut& o, uint32_t max_length = kIdaMaxT) {
        out = o;
        bound = max_length < kIdaMaxT ? max_length : kIdaMaxT;
        max_nodes = nodes;
        total = prev = 0;
        T = h_root;
        it = 0;
        active = false;
        *out.status = DCA_IDASTAR_UNSOLVABLE;
        *out.length = 0;
        *out.num_thresholds = 0;
        *out.total_nodes = 0;
        if (root_goal && !root_dead) *out.status = DCA_IDASTAR_SOLVED;
        if (!root_dead && !root_goal) enter();  // (dead: a table says the goal cannot be reached from the root)
    }
    // Threshold T is to run if it is within the bound; above the caller's bound the search ends as "no solution that short".
    void enter() {
        active = T <= bound;
        if (!active && T <= kIdaMaxT) *out.status = DCA_IDASTAR_BOUNDED;
    }
    unsigned long long budget() const { return (unsigned long long)(max_nodes - total); }
    // Takes threshold T's control block: totals, status, and the next T or the end.
    void step(const IdaCtrl& ctrl) {
        prev = (int64_t)ctrl.nodes;
        total += prev;
        if (it < out.thresholds_cap) {
            out.thresholds[it] = (int)T;
            out.nodes_per_threshold[it] = prev;
        }
        *out.num_thresholds = ++it;
        *out.total_nodes = total;
        active = false;
        if (ctrl.stop & kIdaSolved) {
            *out.status = DCA_IDASTAR_SOLVED;
            *out.length = (int)ctrl.length;
            for (int d = 0; d < (int)ctrl.length && d < out.moves_cap; d++) out.moves[d] = ctrl.moves[d];
            return;
        }
        if ((ctrl.stop & kIdaBudget) || total >= max_nodes) {
            *out.status = DCA_IDASTAR_BUDGET;
            return;
        }
        if (ctrl.best == 0u) return;  // no child above the threshold: the whole space was searched
        T = 0xFFFFFFFFu - ctrl.best;
        enter();
    }
};

// The threshold loop of one root.  run(T, P, n_items, budget, ctrl) runs one iteration and fills `ctrl` (host copy).
template <typename D, typename Run>
static int ida_drive(uint32_t h_root, bool root_dead, bool root_goal, int64_t max_nodes, const IdaOut& out, Run run) {
    IdaRun r;
    for (r.begin(h_root, root_dead, root_goal, max_nodes, out); r.active;) {
        const uint32_t P = ida_prefix<D>(r.prev);
        IdaCtrl ctrl{};
        if (int rc = run(r.T, P, ida_items<D>(P), r.budget(), ctrl)) return rc;
        r.step(ctrl);
    }
    return 0;
}

static int ida_check_out(const char* who, int64_t max_nodes, const IdaOut& o) {
    if (max_nodes <= 0) {
        set_error("bad argument: %s: max_nodes = %lld is not positive", who, (long long)max_nodes);
        return DCA_E_BADARG;
    }
    if (!o.status || !o.length || !o.num_thresholds || !o.total_nodes) {
        set_error("bad argument: %s: status, length, num_thresholds and total_nodes must not be NULL", who);
        return DCA_E_BADARG;
    }
    if (o.moves_cap < 0 || (o.moves_cap > 0 && !o.moves)) {
        set_error("bad argument: %s: moves: NULL with moves_cap = %d", who, o.moves_cap);
        return DCA_E_BADARG;
    }
    if (o.thresholds_cap < 0 || (o.thresholds_cap > 0 && (!o.thresholds || !o.nodes_per_threshold))) {
        set_error("bad argument: %s: thresholds / nodes_per_threshold: NULL with thresholds_cap = %d", who, o.thresholds_cap);
        return DCA_E_BADARG;
    }
    return 0;
}

// the root's bytes: a permutation of 0..N-1 of the goal's parity, or a refusal that names it as `what`
static int ida_check_puzzle_root(const char* who, int dim, const uint8_t* root, const char* what = "root") {
    const int N = dim * dim;
    uint64_t seen = 0;
    int blank = 0;
    for (int i = 0; i < N; i++) {
        const int t = root[i];
        if (t >= N) {
            set_error("bad argument: %s: %s: byte %d at position %d is not a tile of a %d x %d board", who, what, t, i, dim, dim);
            return DCA_E_BADARG;
        }
        if ((seen >> t) & 1) {
            set_error("bad argument: %s: %s: tile %d appears twice", who, what, t);
            return DCA_E_BADARG;
        }
        seen |= 1ull << t;
        if (t == 0) blank = i;
    }
    int inv = 0;
    for (int i = 0; i < N; i++)
        for (int j = i + 1; j < N; j++) inv += root[i] != 0 && root[j] != 0 && root[i] > root[j];
    // a horizontal blank move keeps the tiles' order; a vertical one carries a tile past dim - 1 others
    const int parity = (inv + (dim % 2 == 0 ? dim - 1 - blank / dim : 0)) & 1;
    if (parity) {
        set_error("bad argument: %s: %s: the permutation has the wrong parity, the goal cannot be reached from it", who, what);
        return DCA_E_BADARG;
    }
    return 0;
}

static int ida_check_cube3_root(const char* who, const uint8_t* root, const char* what = "root") {
    uint64_t seen = 0;
    for (int i = 0; i < 54; i++) {
        const int t = root[i];
        if (t >= 54 || ((seen >> t) & 1)) {
            set_error("bad argument: %s: %s: byte %d at position %d: the 54 bytes are not the sticker ids 0..53 once each", who, what, t, i);
            return DCA_E_BADARG;
        }
        seen |= 1ull << t;
    }
    return 0;
}

// a root's 54 sticker ids as the search's state: the two location words
static C3Domain::State c3_root_state(const uint8_t* root) {
    uint32_t w[14];
    pdb_load_row<54, 1>(root, w);
    return {c3_row_locs<DCA_CUBE3_CORNERS, DCA_ROWS_STATE>(w), c3_row_locs<DCA_CUBE3_EDGES, DCA_ROWS_STATE>(w)};
}

// The dual search inverts a lane's words in the or-only form (c3_inverse_locs), which needs every cubie of a kind in a slot of
// its own.  54 distinct sticker ids need not be that (a corner's sticker on an edge): such a root is no cube state — no move
// sequence takes it to the goal — and is refused.  The moves permute the slots, so the root's property is every node's.
static int ida_check_cube3_slots(const char* who, const uint8_t* root, const char* what = "root") {
    const C3Domain::State s0 = c3_root_state(root);
    const uint64_t locs[2] = {s0.corner, s0.edge};
    for (int kind = 0; kind < 2; kind++) {
        const int n = kind == DCA_CUBE3_CORNERS ? 8 : 12, o = kind == DCA_CUBE3_CORNERS ? 3 : 2;
        uint32_t seen = 0;
        for (int q = 0; q < n; q++) seen |= 1u << (((locs[kind] >> (5 * q)) & 31u) / o);
        if (seen != (1u << n) - 1u) {
            set_error("bad argument: %s: %s: the stickers are no cube state: two %s cubies in one slot", who, what,
                      kind == DCA_CUBE3_CORNERS ? "corner" : "edge");
            return DCA_E_BADARG;
        }
    }
    return 0;
}

static int ida_blocks(uint32_t n_items) {
    static int cap = 0;  // (the same value whoever writes it)
    if (cap == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
            cus = 1;
        cap = cus * kIdaBlocksPerCu < kIdaMaxBlocks ? cus * kIdaBlocksPerCu : kIdaMaxBlocks;
    }
    const uint32_t b = (n_items + kIdaThreads - 1) / kIdaThreads;
    return (int)(b < (uint32_t)cap ? b : (uint32_t)cap);
}

// queues the copies of one root's table bytes out of device memory; the caller synchronises, after a failure too
static hipError_t ida_root_bytes_queue(int np, const uint8_t* const* table, const uint64_t* idx, hipStream_t st, uint8_t* v) {
    hipError_t e = hipSuccess;
    for (int p = 0; p < np && e == hipSuccess; p++) e = hipMemcpyAsync(v + p, table[p] + idx[p], 1, hipMemcpyDeviceToHost, st);
    return e;
}

// The root's table bytes, v[p] = table[p][idx[p]]: device memory (the copies queued, then one synchronise) or host memory.
static int ida_root_bytes(bool on_device, int np, const uint8_t* const* table, const uint64_t* idx, hipStream_t st, uint8_t* v) {
    if (!on_device) {
        for (int p = 0; p < np; p++) v[p] = table[p][idx[p]];
        return 0;
    }
    hipError_t e = ida_root_bytes_queue(np, table, idx, st, v);
    const hipError_t sync = hipStreamSynchronize(st);  // also after a failure: no copy into v is left pending
    if (e == hipSuccess) e = sync;
    return e == hipSuccess ? 0 : hip_fail(e, "IDA*: the root's table bytes");
}

// A search's control block.  hipFree synchronises the device, so a search that ends well leaves its block in a one-entry slot
// and the next search on that device takes it from there.  A search holds its block alone: two searches at once (two host
// threads) find the slot empty for one of them, which allocates its own and frees it where the slot is full again.  A search
// that ends on an error frees its block (a launch may still be writing it; the free waits for it).
static std::mutex g_ida_slot_mutex;
static IdaCtrl* g_ida_slot = nullptr;
static int g_ida_slot_device = -1;

static int ida_block_take(IdaCtrl*& block, int& device) {
    DCA_HIP(hipGetDevice(&device));
    {
        std::lock_guard<std::mutex> lock(g_ida_slot_mutex);
        if (g_ida_slot != nullptr && g_ida_slot_device == device) {
            block = g_ida_slot;
            g_ida_slot = nullptr;
            return 0;
        }
    }
    DCA_HIP(hipMalloc((void**)&block, sizeof(IdaCtrl)));
    return 0;
}

static void ida_block_give(IdaCtrl* block, int device, bool idle) {
    if (block == nullptr) return;
    if (idle) {
        std::lock_guard<std::mutex> lock(g_ida_slot_mutex);
        if (g_ida_slot == nullptr) {
            g_ida_slot = block;
            g_ida_slot_device = device;
            return;
        }
    }
    (void)hipFree(block);
}

// One iteration on the device: zero the block, launch, read the block back (this synchronises the stream).
template <typename Launch>
static int ida_device_iteration(IdaCtrl* dev, IdaCtrl& ctrl, hipStream_t st, const char* name, Launch launch) {
    DCA_HIP(hipMemsetAsync(dev, 0, sizeof(IdaCtrl), st));
    launch();
    if (int rc = launch_check(name)) return rc;
    DCA_HIP(hipMemcpyAsync(&ctrl, dev, sizeof(IdaCtrl), hipMemcpyDeviceToHost, st));
    DCA_HIP(hipStreamSynchronize(st));
    return 0;
}

constexpr int kIdaMaxReads = 2 * kC3SymMaxLookups;  // the root's table bytes: the dual search's two passes over a full list

// The frame every search shares, over its domain D.  root: the root's state; reads, tables, idx: the root's table bytes to
// read; reduce(v, reads): the family's h of the root from those bytes (any byte >= 0xFE: the root is dead, whatever the family);
// arg: the kernel's argument as the host lane reads it (D::device_arg makes its device memory, in a copy the launches get);
// maps: what D::ctx takes beside it on the host; launch(arg, blocks, ctrl, T, P, n_items, budget, poll): the family's kernel.
// The order of the HIP calls: the root's bytes, the argument's device memory and a control block — both only where a search
// will run on the device — and per threshold a device iteration (or the host lane); then the block goes back or is freed.
template <typename D, typename Maps, typename Reduce, typename Launch>
static int ida_search(const typename D::State& root, int reads, const uint8_t* const* tables, const uint64_t* idx, Reduce reduce,
                      const typename D::Arg& arg, const Maps& maps, Launch launch, int64_t max_nodes, const IdaOut& out, bool on_device,
                      hipStream_t st) {
    uint8_t v[kIdaMaxReads] = {};
    if (int rc = ida_root_bytes(on_device, reads, tables, idx, st, v)) return rc;
    bool dead = false;
    for (int p = 0; p < reads; p++) dead = dead || v[p] >= kPdbInf;
    const uint32_t h_root = reduce(v, reads);
    const bool goal = D::goal(root);
    typename D::Arg dev_arg = arg;
    IdaCtrl* dev = nullptr;
    int device = -1;
    if (on_device && !dead && !goal) {
        if (int rc = D::device_arg(dev_arg)) return rc;
        if (int rc = ida_block_take(dev, device)) return rc;
    }
    const int rc = ida_drive<D>(h_root, dead, goal, max_nodes, out, [&](uint32_t T, uint32_t P, uint32_t n_items, unsigned long long budget, IdaCtrl& ctrl) {
        if (on_device)
            return ida_device_iteration(dev, ctrl, st, D::kernel_name, [&] {
                launch(dev_arg, dim3(ida_blocks(n_items)), dev, T, P, n_items, budget, ida_poll(budget, ida_blocks(n_items) * kIdaThreads));
            });
        uint32_t stk[D::STACK_WORDS] = {};
        ida_lane<D>(D::ctx(maps, arg), root, &ctrl, stk, 1u, T, P, n_items, budget, ida_poll(budget, 1));
        return 0;
    });
    ida_block_give(dev, device, rc == 0);
    return rc;
}

// A pattern set and one root's bytes as the search reads them: the tile maps and the table slots (the set's alone, whatever
// the root), and the root's state with the table index of each of its `reads` root bytes.
template <int DIM, bool REFLECT>
static void pz_prepare(const uint8_t* root, const PdbSet& set, PzMapsOf<REFLECT>& maps, PzArgs<DIM, REFLECT>& args, uint64_t* root_idx) {
    using D = PzDomain<DIM, REFLECT>;
    constexpr int N = D::N;
    maps = {};
    for (int t = 0; t < 32; t++) maps.p[t] = 0xFFu;
    if constexpr (REFLECT)
        for (int t = 0; t < 32; t++) maps.rp[t] = 0xFFu;
    args = {};
    args.np = set.np;
    int pos[N];
    for (int i = 0; i < N; i++) {
        pos[root[i]] = i;
        args.root.board |= (typename D::Board)root[i] << (D::BITS * i);
    }
    args.root.blank = (uint32_t)pos[0];
    for (int p = 0; p < set.np; p++) {
        uint64_t w = N;  // the blank is digit 0, tiles[j] digit j + 1
        for (int j = 0; j < set.k[p]; j++, w *= N) {
            const int t = set.pat[p].id[j];
            maps.w[t] = w;
            maps.p[t] = (uint32_t)p;
            args.root.idx[p] += w * (uint64_t)pos[t];
            if constexpr (REFLECT) {  // slot np + p: tile t's digit in the mirror image is refl(pos(phi(t))); phi(t) moves it
                const int u = (int)pdb_phi<DIM>((uint32_t)t);
                maps.rw[u] = w;
                maps.rp[u] = (uint32_t)(set.np + p);
                args.root.idx[set.np + p] += w * (uint64_t)pdb_refl<DIM>((uint32_t)pos[u]);
            }
        }
        args.table[p] = set.table[p];
        root_idx[p] = args.root.idx[p] + args.root.blank;
        if constexpr (REFLECT) {
            args.table[set.np + p] = set.table[p];
            root_idx[set.np + p] = args.root.idx[set.np + p] + pdb_refl<DIM>(args.root.blank);
        }
    }
}

// h of a puzzle root from its bytes: the patterns' sum, or the larger of it and the mirror image's
static uint32_t pz_larger_sum(const uint8_t* v, int slots, int np) {
    uint32_t h_root = 0, h_mirror = 0;
    for (int p = 0; p < slots; p++) (p < np ? h_root : h_mirror) += v[p];
    return h_root > h_mirror ? h_root : h_mirror;
}

template <int DIM, bool REFLECT>
static int ida_puzzle(const uint8_t* root, const PdbSet& set, int64_t max_nodes, const IdaOut& out, bool on_device, hipStream_t st) {
    using D = PzDomain<DIM, REFLECT>;
    PzMapsOf<REFLECT> maps;
    PzArgs<DIM, REFLECT> args;
    uint64_t root_idx[kIdaPuzzlePatterns] = {};
    pz_prepare<DIM, REFLECT>(root, set, maps, args, root_idx);
    const auto larger_sum = [&](const uint8_t* v, int slots) { return pz_larger_sum(v, slots, set.np); };
    return ida_search<D>(
        args.root, REFLECT ? 2 * set.np : set.np, args.table, root_idx, larger_sum, args, maps,
        [&](const PzArgs<DIM, REFLECT>& arg, dim3 blocks, IdaCtrl* ctrl, uint32_t T, uint32_t P, uint32_t n_items, unsigned long long budget, uint32_t poll) {
            hipLaunchKernelGGL((ida_puzzle_kernel<DIM, REFLECT>), blocks, dim3(kIdaThreads), 0, st, arg, maps, ctrl, T, P, n_items, budget, poll);
        },
        max_nodes, out, on_device, st);
}

// root r's outputs out of the batch's arrays
static IdaOut ida_out_at(const IdaOut& o, int r) {
    const size_t m = (size_t)r * (size_t)o.moves_cap, t = (size_t)r * (size_t)o.thresholds_cap;
    return {o.status + r, o.length + r, o.moves ? o.moves + m : nullptr, o.moves_cap, o.num_thresholds + r,
            o.thresholds ? o.thresholds + t : nullptr, o.nodes_per_threshold ? o.nodes_per_threshold + t : nullptr, o.thresholds_cap,
            o.total_nodes + r};
}

// The rounds of a batch, whatever the family: every root's IdaRun has begun (state[r] its root, run[r] its run), and a round is
// the next threshold of every root still active, each with the T, P, items, budget, poll interval and blocks its single search
// would give it.  Root: the family's descriptor (PzBatchRoot, C3BatchRoot); c: the host lane's context; launch(dev_desc, n,
// blocks, dev_ctrl): the family's batch kernel on the round's n descriptors.  The order of the HIP calls: the control blocks
// and the descriptors in one allocation; per round one memset of the round's control blocks, one upload of its descriptors,
// one launch, one read-back, one synchronise; the free.  The host twin runs a round's roots one after the other on ida_lane,
// as ida_search does its one root.
// P is the single search's rule on the root's own previous count.  A shallower one for batches — the deepest P whose items
// times the round's roots pass D::worth, fewer items a root wasting less replay — was measured on the puzzles and was slower at
// every batch size (profiles/idastar_batch_probe.txt): the deep prefix is also what balances a round whose roots differ a
// thousandfold.
template <typename D, typename Root, typename Launch>
static int ida_batch_rounds(const typename D::State* state, std::vector<IdaRun>& run, bool on_device, hipStream_t st, const char* name,
                            const typename D::Ctx& c, Launch launch) {
    const int n_roots = (int)run.size();
    std::vector<Root> desc((size_t)n_roots);
    std::vector<IdaCtrl> ctrl((size_t)n_roots);
    std::vector<int> slot((size_t)n_roots);  // the round's j-th root
    constexpr size_t kCtrlBytes = sizeof(IdaCtrl), kRootBytes = sizeof(Root);
    static_assert(kCtrlBytes % 16 == 0, "the descriptors stand behind the control blocks");
    IdaCtrl* dev_ctrl = nullptr;
    if (on_device) DCA_HIP(hipMalloc((void**)&dev_ctrl, (size_t)n_roots * (kCtrlBytes + kRootBytes)));
    Root* dev_desc = on_device ? (Root*)(dev_ctrl + n_roots) : nullptr;
    const auto round = [&](int n, uint32_t blocks) -> int {
        if (!on_device) {
            for (int j = 0; j < n; j++) {
                uint32_t stk[D::STACK_WORDS] = {};
                ctrl[j] = IdaCtrl{};
                ida_lane<D>(c, desc[j].root, &ctrl[j], stk, 1u, desc[j].T, desc[j].P, desc[j].n_items, desc[j].budget, desc[j].poll);
            }
            return 0;
        }
        DCA_HIP(hipMemsetAsync(dev_ctrl, 0, (size_t)n * kCtrlBytes, st));
        DCA_HIP(hipMemcpyAsync(dev_desc, desc.data(), (size_t)n * kRootBytes, hipMemcpyHostToDevice, st));
        launch((const Root*)dev_desc, n, blocks, dev_ctrl);
        if (int rc = launch_check(name)) return rc;
        DCA_HIP(hipMemcpyAsync(ctrl.data(), dev_ctrl, (size_t)n * kCtrlBytes, hipMemcpyDeviceToHost, st));
        DCA_HIP(hipStreamSynchronize(st));
        return 0;
    };
    int rc = 0;
    while (rc == 0) {
        int n = 0;
        uint32_t blocks = 0;
        for (int r = 0; r < n_roots; r++) {
            if (!run[r].active) continue;
            Root& d = desc[n];
            d = Root{};
            d.root = state[r];
            d.budget = run[r].budget();
            d.T = run[r].T;
            d.P = ida_prefix<D>(run[r].prev);
            d.n_items = ida_items<D>(d.P);
            const int own = on_device ? ida_blocks(d.n_items) : 1;
            d.poll = ida_poll(d.budget, on_device ? own * kIdaThreads : 1);
            d.first_block = blocks;
            blocks += (uint32_t)own;
            slot[n++] = r;
        }
        if (n == 0) break;  // every root has left the batch
        rc = round(n, blocks);
        for (int j = 0; j < n && rc == 0; j++) run[slot[j]].step(ctrl[j]);
    }
    if (dev_ctrl != nullptr) (void)hipFree(dev_ctrl);  // (after an error a launch may still be writing: the free waits for it)
    return rc;
}

// A batch of puzzle roots on one pattern set (include/dca.h "batches"): ida_search's frame with an IdaRun per root and
// ida_batch_rounds in place of one root's thresholds.  The HIP calls in front of the rounds: every root's table bytes queued
// and one synchronise.
template <int DIM, bool REFLECT>
static int ida_puzzle_batch(const uint8_t* roots, int n_roots, const PdbSet& set, int64_t max_nodes, const IdaOut& out, bool on_device,
                            hipStream_t st) {
    using D = PzDomain<DIM, REFLECT>;
    using Root = PzBatchRoot<DIM, REFLECT>;
    const int reads = REFLECT ? 2 * set.np : set.np;
    PzMapsOf<REFLECT> maps;
    PzArgs<DIM, REFLECT> args;
    std::vector<typename D::State> state((size_t)n_roots);
    std::vector<uint8_t> v((size_t)n_roots * kIdaPuzzlePatterns);
    hipError_t e = hipSuccess;
    for (int r = 0; r < n_roots; r++) {
        uint64_t root_idx[kIdaPuzzlePatterns] = {};
        pz_prepare<DIM, REFLECT>(roots + (size_t)r * D::N, set, maps, args, root_idx);
        state[r] = args.root;
        uint8_t* bytes = v.data() + (size_t)r * kIdaPuzzlePatterns;
        if (!on_device)
            for (int p = 0; p < reads; p++) bytes[p] = args.table[p][root_idx[p]];
        else if (e == hipSuccess)
            e = ida_root_bytes_queue(reads, args.table, root_idx, st, bytes);
    }
    if (on_device) {
        const hipError_t sync = hipStreamSynchronize(st);  // also after a failure: no copy into v is left pending
        if (e == hipSuccess) e = sync;
        if (e != hipSuccess) return hip_fail(e, "IDA*: the roots' table bytes");
    }
    std::vector<IdaRun> run((size_t)n_roots);
    bool any = false;
    for (int r = 0; r < n_roots; r++) {
        const uint8_t* bytes = v.data() + (size_t)r * kIdaPuzzlePatterns;
        bool dead = false;
        for (int p = 0; p < reads; p++) dead = dead || bytes[p] >= kPdbInf;
        run[r].begin(pz_larger_sum(bytes, reads, set.np), dead, D::goal(state[r]), max_nodes, ida_out_at(out, r));
        any = any || run[r].active;
    }
    if (!any) return 0;
    const typename D::Ctx c = D::ctx(maps, args);
    return ida_batch_rounds<D, Root>(
        state.data(), run, on_device, st, "ida_puzzle_batch_kernel", c, [&](const Root* dev_desc, int n, uint32_t blocks, IdaCtrl* dev_ctrl) {
            PzBatchArgs<DIM, REFLECT> a{};
            a.roots = dev_desc;
            a.n_roots = (uint32_t)n;
            for (int q = 0; q < kIdaPuzzlePatterns; q++) a.table[q] = args.table[q];
            a.np = args.np;
            hipLaunchKernelGGL((ida_puzzle_batch_kernel<DIM, REFLECT>), dim3(blocks), dim3(kIdaThreads), 0, st, a, maps, dev_ctrl);
        });
}

static C3IdaMoves c3_ida_moves() {
    C3IdaMoves mt{};
    for (int kind = 0; kind < 2; kind++)
        for (int a = 0; a < 12; a++)
            for (int l = 0; l < kC3Locs; l++)
                mt.w[((kind * 12 + a) * kC3Locs + l) >> 2] |= (uint32_t)kC3.move[kind][a][l] << (8 * (l & 3));
    return mt;
}

// A cube3 search of any family from its root, the root's reads and its argument: h of the root is the largest byte.
template <typename D>
static int ida_cube3_search(const C3Domain::State& s0, int reads, const uint8_t* const* tables, const uint64_t* idx, const typename D::Arg& arg,
                            int64_t max_nodes, const IdaOut& out, bool on_device, hipStream_t st) {
    const C3IdaMoves mt = c3_ida_moves();
    const auto largest = [](const uint8_t* v, int n) {
        uint32_t h_root = 0;
        for (int p = 0; p < n; p++) h_root = h_root > v[p] ? h_root : v[p];
        return h_root;
    };
    return ida_search<D>(
        s0, reads, tables, idx, largest, arg, (const uint8_t*)mt.w,  // little-endian words: byte l of a row is location l
        [&](const typename D::Arg& a, dim3 blocks, IdaCtrl* ctrl, uint32_t T, uint32_t P, uint32_t n_items, unsigned long long budget, uint32_t poll) {
            hipLaunchKernelGGL(ida_cube3_kernel<D>, blocks, dim3(kIdaThreads), 0, st, s0, a, mt, ctrl, T, P, n_items, budget, poll);
        },
        max_nodes, out, on_device, st);
}

// The reads of a look-up list at a root -> their number: the root's h is the full maximum, and the root is dead where ANY
// look-up's byte is >= 0xFE.  dual: the root's bytes are those of the list at the state and, behind them, those of the second
// pass at the inverse state (every look-up that does not name all the cubies of its kind).
static int c3_list_reads(const C3Domain::State& s0, const C3SymList& list, bool dual, const uint8_t** tables, uint64_t* root_idx) {
    int reads = 0;
    for (int p = 0; p < list.n; p++, reads++) {
        const C3Lookup& lk = list.lk[p];
        root_idx[reads] = c3_sym_index(&lk, c3_lookup_head(&lk), s0.corner, s0.edge);
        tables[reads] = lk.table;
    }
    if (dual) {
        const uint64_t corner = c3_inverse_locs<DCA_CUBE3_CORNERS, false>(s0.corner), edge = c3_inverse_locs<DCA_CUBE3_EDGES, false>(s0.edge);
        for (int p = 0; p < list.n; p++) {
            const C3Lookup& lk = list.lk[p];
            if (c3_lookup_whole(c3_lookup_head(&lk))) continue;
            root_idx[reads] = c3_sym_index(&lk, c3_lookup_head(&lk), corner, edge);
            tables[reads++] = lk.table;
        }
    }
    return reads;
}

// The search on the symmetric look-ups: ida_cube3 with the list in place of the set.  The list's tables are device memory
// (on_device) or host memory.  dual: the search on the dual look-ups.
static int ida_cube3_sym(const uint8_t* root, const C3SymList& list, int64_t max_nodes, const IdaOut& out, bool on_device, hipStream_t st,
                         bool dual = false) {
    const C3Domain::State s0 = c3_root_state(root);
    uint64_t root_idx[kIdaMaxReads] = {};
    const uint8_t* tables[kIdaMaxReads] = {};
    const int reads = c3_list_reads(s0, list, dual, tables, root_idx);
    C3DualSet arg;
    c3_list_arg(list, arg);
    return dual ? ida_cube3_search<C3DualDomain>(s0, reads, tables, root_idx, arg, max_nodes, out, on_device, st)
                : ida_cube3_search<C3SymDomain>(s0, reads, tables, root_idx, arg, max_nodes, out, on_device, st);
}

// the plain search's reads at a root: one byte a pattern
static int c3_set_reads(const C3Domain::State& s0, const C3Set& set, const uint8_t** tables, uint64_t* root_idx) {
    for (int p = 0; p < set.np; p++) {
        root_idx[p] = set.kind[p] == DCA_CUBE3_CORNERS ? c3_index<DCA_CUBE3_CORNERS>(s0.corner, set.pat[p], set.k[p])
                                                      : c3_index<DCA_CUBE3_EDGES>(s0.edge, set.pat[p], set.k[p]);
        tables[p] = set.table[p];
    }
    return set.np;
}

static int ida_cube3(const uint8_t* root, const C3Set& set, int64_t max_nodes, const IdaOut& out, bool on_device, hipStream_t st) {
    const C3Domain::State s0 = c3_root_state(root);
    uint64_t root_idx[kPdbMaxPatterns] = {};
    const uint8_t* tables[kPdbMaxPatterns] = {};
    const int reads = c3_set_reads(s0, set, tables, root_idx);
    return ida_cube3_search<C3Domain>(s0, reads, tables, root_idx, set, max_nodes, out, on_device, st);
}

// A batch of cube3 roots on one pattern set and look-up mode (include/dca.h "bounded batches"): ida_puzzle_batch's frame.  D: the
// mode's domain; arg: its argument as the host lane reads it (D::device_arg makes its device memory once, and only where a
// root will search on the device); reads_of(s0, tables, idx): the mode's reads at a root, whose largest byte is h of the root
// and of which any >= 0xFE makes it dead; bound: the roots' bounds or NULL.
template <typename D, typename Reads>
static int ida_cube3_batch(const uint8_t* roots, int n_roots, const typename D::Arg& arg, Reads reads_of, const int* bound, int64_t max_nodes,
                           const IdaOut& out, bool on_device, hipStream_t st) {
    std::vector<C3Domain::State> state((size_t)n_roots);
    std::vector<uint8_t> v((size_t)n_roots * kIdaMaxReads);
    std::vector<int> reads((size_t)n_roots);
    hipError_t e = hipSuccess;
    for (int r = 0; r < n_roots; r++) {
        uint64_t root_idx[kIdaMaxReads] = {};
        const uint8_t* tables[kIdaMaxReads] = {};
        state[r] = c3_root_state(roots + (size_t)r * 54);
        reads[r] = reads_of(state[r], tables, root_idx);
        uint8_t* bytes = v.data() + (size_t)r * kIdaMaxReads;
        if (!on_device)
            for (int p = 0; p < reads[r]; p++) bytes[p] = tables[p][root_idx[p]];
        else if (e == hipSuccess)
            e = ida_root_bytes_queue(reads[r], tables, root_idx, st, bytes);
    }
    if (on_device) {
        const hipError_t sync = hipStreamSynchronize(st);  // also after a failure: no copy into v is left pending
        if (e == hipSuccess) e = sync;
        if (e != hipSuccess) return hip_fail(e, "IDA*: the roots' table bytes");
    }
    std::vector<IdaRun> run((size_t)n_roots);
    bool any = false;
    for (int r = 0; r < n_roots; r++) {
        const uint8_t* bytes = v.data() + (size_t)r * kIdaMaxReads;
        bool dead = false;
        uint32_t h_root = 0;
        for (int p = 0; p < reads[r]; p++) {
            dead = dead || bytes[p] >= kPdbInf;
            h_root = h_root > bytes[p] ? h_root : bytes[p];
        }
        run[r].begin(h_root, dead, C3Domain::goal(state[r]), max_nodes, ida_out_at(out, r), bound ? (uint32_t)bound[r] : kIdaMaxT);
        any = any || run[r].active;
    }
    if (!any) return 0;
    const C3IdaMoves mt = c3_ida_moves();
    typename D::Arg dev_arg = arg;
    if (on_device)
        if (int rc = D::device_arg(dev_arg)) return rc;
    return ida_batch_rounds<D, C3BatchRoot>(
        state.data(), run, on_device, st, "ida_cube3_batch_kernel", D::ctx((const uint8_t*)mt.w, arg),
        [&](const C3BatchRoot* dev_desc, int n, uint32_t blocks, IdaCtrl* dev_ctrl) {
            hipLaunchKernelGGL(ida_cube3_batch_kernel<D>, dim3(blocks), dim3(kIdaThreads), 0, st, dev_desc, (uint32_t)n, dev_arg, mt, dev_ctrl);
        });
}

// every refusal of a puzzle search but the root's own (root: the root, or a batch's roots), and the pattern set
static int ida_npuzzle_set(const char* who, int dim, const uint8_t* root, int num_patterns, const uint8_t* tiles, const int* ks,
                           const uint8_t* const* tables, int64_t max_nodes, const IdaOut& out, bool reflect, PdbSet& set) {
    if (dim < 3 || dim > 7) {
        set_error("bad argument: %s: dim: unsupported puzzle dim %d (3..5)", who, dim);
        return DCA_E_BADARG;
    }
    if (dim > 5) {
        set_error("bad argument: %s: dim: IDA* is built for dim 3..5; an optimal solution of a %d x %d board is out of reach", who, dim, dim);
        return DCA_E_BADARG;
    }
    if (root == nullptr || tiles == nullptr || ks == nullptr || tables == nullptr) {
        set_error("bad argument: %s: root, tiles, ks and tables must not be NULL", who);
        return DCA_E_BADARG;
    }
    if (num_patterns < 1 || num_patterns > kIdaPuzzlePatterns) {
        set_error("bad argument: %s: num_patterns = %d is not in 1..%d (a lane keeps one running index per pattern)", who, num_patterns,
                  kIdaPuzzlePatterns);
        return DCA_E_BADARG;
    }
    if (reflect && num_patterns > kIdaPuzzlePatterns / 2) {
        set_error("bad argument: %s: num_patterns = %d is not in 1..%d (a lane keeps a running index and a reflected one per pattern, %d in all)",
                  who, num_patterns, kIdaPuzzlePatterns / 2, kIdaPuzzlePatterns);
        return DCA_E_BADARG;
    }
    if (int rc = ida_check_out(who, max_nodes, out)) return rc;
    const int N = dim * dim;
    set = {};
    uint64_t seen = 0;
    return pdb_fill_set(
        who, set, num_patterns, tiles, ks, tables, [&](int p) { return pdb_bytes_checked(who, dim, ks[p]); },
        [&](int p, const uint8_t* t) {
            if (ks[p] > kPdbMaxK) {
                set_error("bad argument: %s: ks: pattern %d has %d tiles, over %d", who, p, ks[p], kPdbMaxK);
                return DCA_E_BADARG;
            }
            return pdb_check_tiles(who, N, t, ks[p], seen);
        });
}

// every refusal of a puzzle search, then the search: before any HIP call
static int ida_npuzzle_entry(const char* who, int dim, const uint8_t* root, int num_patterns, const uint8_t* tiles, const int* ks,
                             const uint8_t* const* tables, int64_t max_nodes, const IdaOut& out, bool on_device, hipStream_t st,
                             bool reflect = false) {
    PdbSet set;
    if (int rc = ida_npuzzle_set(who, dim, root, num_patterns, tiles, ks, tables, max_nodes, out, reflect, set)) return rc;
    if (int rc = ida_check_puzzle_root(who, dim, root)) return rc;
    if (reflect)
        switch (dim) {
            case 3: return ida_puzzle<3, true>(root, set, max_nodes, out, on_device, st);
            case 4: return ida_puzzle<4, true>(root, set, max_nodes, out, on_device, st);
            default: return ida_puzzle<5, true>(root, set, max_nodes, out, on_device, st);
        }
    switch (dim) {
        case 3: return ida_puzzle<3, false>(root, set, max_nodes, out, on_device, st);
        case 4: return ida_puzzle<4, false>(root, set, max_nodes, out, on_device, st);
        default: return ida_puzzle<5, false>(root, set, max_nodes, out, on_device, st);
    }
}

// every refusal of a batch of puzzle searches, a bad root by its index, then the batch: before any HIP call and any output
static int ida_npuzzle_batch_entry(const char* who, int dim, const uint8_t* roots, int n_roots, int num_patterns, const uint8_t* tiles,
                                   const int* ks, const uint8_t* const* tables, bool reflect, int64_t max_nodes, const IdaOut& out,
                                   bool on_device, hipStream_t st) {
    if (n_roots < 1 || n_roots > DCA_IDASTAR_MAX_BATCH) {
        set_error("bad argument: %s: n_roots = %d is not in 1..%d", who, n_roots, DCA_IDASTAR_MAX_BATCH);
        return DCA_E_BADARG;
    }
    PdbSet set;
    if (int rc = ida_npuzzle_set(who, dim, roots, num_patterns, tiles, ks, tables, max_nodes, out, reflect, set)) return rc;
    for (int r = 0; r < n_roots; r++) {
        char what[32];
        snprintf(what, sizeof(what), "roots[%d]", r);
        if (int rc = ida_check_puzzle_root(who, dim, roots + (size_t)r * (size_t)(dim * dim), what)) return rc;
    }
    if (reflect)
        switch (dim) {
            case 3: return ida_puzzle_batch<3, true>(roots, n_roots, set, max_nodes, out, on_device, st);
            case 4: return ida_puzzle_batch<4, true>(roots, n_roots, set, max_nodes, out, on_device, st);
            default: return ida_puzzle_batch<5, true>(roots, n_roots, set, max_nodes, out, on_device, st);
        }
    switch (dim) {
        case 3: return ida_puzzle_batch<3, false>(roots, n_roots, set, max_nodes, out, on_device, st);
        case 4: return ida_puzzle_batch<4, false>(roots, n_roots, set, max_nodes, out, on_device, st);
        default: return ida_puzzle_batch<5, false>(roots, n_roots, set, max_nodes, out, on_device, st);
    }
}

static int ida_cube3_entry(const char* who, const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                           const uint8_t* const* tables, int64_t max_nodes, const IdaOut& out, bool on_device, hipStream_t st) {
    if (root == nullptr || kinds == nullptr || cubies == nullptr || ks == nullptr || tables == nullptr) {
        set_error("bad argument: %s: root, kinds, cubies, ks and tables must not be NULL", who);
        return DCA_E_BADARG;
    }
    if (num_patterns < 1 || num_patterns > kPdbMaxPatterns) {
        set_error("bad argument: %s: num_patterns = %d is not in 1..%d", who, num_patterns, kPdbMaxPatterns);
        return DCA_E_BADARG;
    }
    if (int rc = ida_check_out(who, max_nodes, out)) return rc;
    C3Set set{};
    if (int rc = c3_fill_set(who, num_patterns, kinds, cubies, ks, tables, set)) return rc;
    if (int rc = ida_check_cube3_root(who, root)) return rc;
    return ida_cube3(root, set, max_nodes, out, on_device, st);
}

// every refusal of a symmetric cube3 search, then the search: before any HIP call
static int ida_cube3_sym_entry(const char* who, const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                               const uint8_t* const* tables, int max_images, int64_t max_nodes, const IdaOut& out, bool on_device,
                               hipStream_t st, bool dual = false) {
    if (root == nullptr) {
        set_error("bad argument: %s: root must not be NULL", who);
        return DCA_E_BADARG;
    }
    if (int rc = ida_check_out(who, max_nodes, out)) return rc;
    C3Set set{};
    C3SymList list;
    if (int rc = c3_fill_sym_entry(who, num_patterns, kinds, cubies, ks, tables, max_images, set, list)) return rc;
    if (int rc = ida_check_cube3_root(who, root)) return rc;
    if (dual)
        if (int rc = ida_check_cube3_slots(who, root)) return rc;
    return ida_cube3_sym(root, list, max_nodes, out, on_device, st, dual);
}

// every refusal of a bounded batch of cube3 searches, a bad root by its index, then the batch: before any HIP call and any
// output.  max_images = 0: the plain search; otherwise the symmetric one, or (dual) the dual one.
static int ida_cube3_batch_entry(const char* who, const uint8_t* roots, int n_roots, int num_patterns, const int* kinds, const uint8_t* cubies,
                                 const int* ks, const uint8_t* const* tables, int max_images, bool dual, const int* max_length,
                                 int64_t max_nodes, const IdaOut& out, bool on_device, hipStream_t st) {
    if (n_roots < 1 || n_roots > DCA_IDASTAR_MAX_BATCH) {
        set_error("bad argument: %s: n_roots = %d is not in 1..%d", who, n_roots, DCA_IDASTAR_MAX_BATCH);
        return DCA_E_BADARG;
    }
    if (roots == nullptr) {
        set_error("bad argument: %s: roots must not be NULL", who);
        return DCA_E_BADARG;
    }
    if (int rc = ida_check_out(who, max_nodes, out)) return rc;
    const bool plain = max_images == 0 && !dual;
    C3Set set{};
    C3SymList list;
    if (int rc = c3_fill_sym_entry(who, num_patterns, kinds, cubies, ks, tables, plain ? 1 : max_images, set, list)) return rc;
    for (int r = 0; r < n_roots; r++) {
        char what[32];
        snprintf(what, sizeof(what), "roots[%d]", r);
        if (max_length != nullptr && max_length[r] < 0) {
            set_error("bad argument: %s: max_length[%d] = %d is negative", who, r, max_length[r]);
            return DCA_E_BADARG;
        }
        if (int rc = ida_check_cube3_root(who, roots + (size_t)r * 54, what)) return rc;
        if (dual)
            if (int rc = ida_check_cube3_slots(who, roots + (size_t)r * 54, what)) return rc;
    }
    if (plain)
        return ida_cube3_batch<C3Domain>(
            roots, n_roots, set, [&](const C3Domain::State& s0, const uint8_t** t, uint64_t* idx) { return c3_set_reads(s0, set, t, idx); }, max_length,
            max_nodes, out, on_device, st);
    C3DualSet arg;
    c3_list_arg(list, arg);
    const auto reads_of = [&](const C3Domain::State& s0, const uint8_t** t, uint64_t* idx) { return c3_list_reads(s0, list, dual, t, idx); };
    return dual ? ida_cube3_batch<C3DualDomain>(roots, n_roots, arg, reads_of, max_length, max_nodes, out, on_device, st)
                : ida_cube3_batch<C3SymDomain>(roots, n_roots, arg, reads_of, max_length, max_nodes, out, on_device, st);
}

}  // namespace dca

using namespace dca;

extern "C" {

int dca_idastar_npuzzle(int dim, const uint8_t* root, int num_patterns, const uint8_t* tiles, const int* ks, const uint8_t* const* tables,
                        int64_t max_nodes, int* status, int* length, uint8_t* moves, int moves_cap, int* num_thresholds, int* thresholds,
                        int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes, void* stream) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_npuzzle_entry(__func__, dim, root, num_patterns, tiles, ks, tables, max_nodes, out, true, (hipStream_t)stream);
}

int dca_idastar_npuzzle_reflected(int dim, const uint8_t* root, int num_patterns, const uint8_t* tiles, const int* ks,
                                  const uint8_t* const* tables, int64_t max_nodes, int* status, int* length, uint8_t* moves, int moves_cap,
                                  int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap,
                                  int64_t* total_nodes, void* stream) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_npuzzle_entry(__func__, dim, root, num_patterns, tiles, ks, tables, max_nodes, out, true, (hipStream_t)stream, true);
}

int dca_idastar_npuzzle_batch(int dim, const uint8_t* roots, int n_roots, int num_patterns, const uint8_t* tiles, const int* ks,
                              const uint8_t* const* tables, int reflect, int64_t max_nodes, int* status, int* length, uint8_t* moves,
                              int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap,
                              int64_t* total_nodes, void* stream) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_npuzzle_batch_entry(__func__, dim, roots, n_roots, num_patterns, tiles, ks, tables, reflect != 0, max_nodes, out, true,
                                   (hipStream_t)stream);
}

int dca_idastar_host_batch(int dim, const uint8_t* roots, int n_roots, int num_patterns, const uint8_t* tiles, const int* ks,
                           const uint8_t* const* tables, int reflect, int64_t max_nodes, int* status, int* length, uint8_t* moves,
                           int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap,
                           int64_t* total_nodes) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_npuzzle_batch_entry(__func__, dim, roots, n_roots, num_patterns, tiles, ks, tables, reflect != 0, max_nodes, out, false,
                                   nullptr);
}

int dca_idastar_cube3(const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                      const uint8_t* const* tables, int64_t max_nodes, int* status, int* length, uint8_t* moves, int moves_cap,
                      int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes,
                      void* stream) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_cube3_entry(__func__, root, num_patterns, kinds, cubies, ks, tables, max_nodes, out, true, (hipStream_t)stream);
}

int dca_idastar_cube3_sym(const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                          const uint8_t* const* tables, int max_images, int64_t max_nodes, int* status, int* length, uint8_t* moves,
                          int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap,
                          int64_t* total_nodes, void* stream) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_cube3_sym_entry(__func__, root, num_patterns, kinds, cubies, ks, tables, max_images, max_nodes, out, true, (hipStream_t)stream);
}

int dca_idastar_cube3_dual(const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                           const uint8_t* const* tables, int max_images, int64_t max_nodes, int* status, int* length, uint8_t* moves,
                           int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap,
                           int64_t* total_nodes, void* stream) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_cube3_sym_entry(__func__, root, num_patterns, kinds, cubies, ks, tables, max_images, max_nodes, out, true, (hipStream_t)stream, true);
}

int dca_idastar_cube3_batch(const uint8_t* roots, int n_roots, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                            const uint8_t* const* tables, int max_images, int dual, const int* max_length, int64_t max_nodes, int* status,
                            int* length, uint8_t* moves, int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold,
                            int thresholds_cap, int64_t* total_nodes, void* stream) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_cube3_batch_entry(__func__, roots, n_roots, num_patterns, kinds, cubies, ks, tables, max_images, dual != 0, max_length, max_nodes,
                                 out, true, (hipStream_t)stream);
}

int dca_idastar_host_cube3_batch(const uint8_t* roots, int n_roots, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                                 const uint8_t* const* tables, int max_images, int dual, const int* max_length, int64_t max_nodes,
                                 int* status, int* length, uint8_t* moves, int moves_cap, int* num_thresholds, int* thresholds,
                                 int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_cube3_batch_entry(__func__, roots, n_roots, num_patterns, kinds, cubies, ks, tables, max_images, dual != 0, max_length, max_nodes,
                                 out, false, nullptr);
}

int dca_idastar_host(int env, int dim, const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* ids, const int* ks,
                     const uint8_t* const* tables, int64_t max_nodes, int* status, int* length, uint8_t* moves, int moves_cap,
                     int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    if (env == DCA_ENV_NPUZZLE) return ida_npuzzle_entry(__func__, dim, root, num_patterns, ids, ks, tables, max_nodes, out, false, nullptr);
    if (env == DCA_ENV_CUBE3) return ida_cube3_entry(__func__, root, num_patterns, kinds, ids, ks, tables, max_nodes, out, false, nullptr);
    set_error("bad argument: %s: env = %d is neither cube3 nor a sliding puzzle", __func__, env);
    return DCA_E_BADARG;
}

int dca_idastar_host_reflected(int dim, const uint8_t* root, int num_patterns, const uint8_t* tiles, const int* ks,
                               const uint8_t* const* tables, int64_t max_nodes, int* status, int* length, uint8_t* moves, int moves_cap,
                               int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap, int64_t* total_nodes) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_npuzzle_entry(__func__, dim, root, num_patterns, tiles, ks, tables, max_nodes, out, false, nullptr, true);
}

int dca_idastar_host_sym(const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                         const uint8_t* const* tables, int max_images, int64_t max_nodes, int* status, int* length, uint8_t* moves,
                         int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap,
                         int64_t* total_nodes) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_cube3_sym_entry(__func__, root, num_patterns, kinds, cubies, ks, tables, max_images, max_nodes, out, false, nullptr);
}

int dca_idastar_host_dual(const uint8_t* root, int num_patterns, const int* kinds, const uint8_t* cubies, const int* ks,
                          const uint8_t* const* tables, int max_images, int64_t max_nodes, int* status, int* length, uint8_t* moves,
                          int moves_cap, int* num_thresholds, int* thresholds, int64_t* nodes_per_threshold, int thresholds_cap,
                          int64_t* total_nodes) {
    const IdaOut out{status, length, moves, moves_cap, num_thresholds, thresholds, nodes_per_threshold, thresholds_cap, total_nodes};
    return ida_cube3_sym_entry(__func__, root, num_patterns, kinds, cubies, ks, tables, max_images, max_nodes, out, false, nullptr, true);
}

int dca_idastar_set_prefix(int depth) {
    if (depth < -1 || depth > PzDomain<3>::MAX_PREFIX) {
        set_error("bad argument: %s: depth = %d is not in -1..%d", __func__, depth, (int)PzDomain<3>::MAX_PREFIX);
        return DCA_E_BADARG;
    }
    g_ida_forced_prefix = depth;
    return 0;
}

}  // extern "C"
