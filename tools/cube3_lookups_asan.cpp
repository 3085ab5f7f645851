// The cube3 look-up modes' host code under AddressSanitizer / UBSan, on a CPU (no device is touched, no Python): the kernels'
// own row value through dca_cube3_pdb_eval_sym_host and dca_cube3_pdb_eval_dual_host — rows of cube states and rows of random
// bytes (all 256 values), for 1, 2 and 48 images — and the kernels' search code through dca_idastar_host (cube3),
// dca_idastar_host_sym and dca_idastar_host_dual on a root two moves from the goal, all on exact-size heap tables of zeros (one
// corner pattern of 2 cubies, 504 bytes; one edge pattern of 2 cubies, 528 bytes), so an index past a table or a row is a heap
// overflow here and the search is plain iterative deepening; then those five entry points' refusals, which come before any
// HIP call.  A stand-alone program, so the sanitizer's runtime is linked in, not preloaded:
//
//   cd deepcubea_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I ../../include ../../tools/cube3_lookups_asan.cpp dca_idastar.hip dca_pdb_cube3.hip dca_env.hip -o /tmp/cube3_lookups_asan
//   /tmp/cube3_lookups_asan      # prints "N rows, M searches, K refusals: ok", exit status 0; a sanitizer report otherwise
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dca.h"
#include "dca_debug.h"

static int failures = 0, refusals = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;

static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 24);
}

static void fail(const char* what, long long a = 0, long long b = 0) {
    printf("FAILED: %s (%lld, %lld)\n", what, a, b);
    failures++;
}

static void refused(int rc, const char* who, const char* word) {
    const char* msg = dca_last_error();
    refusals++;
    if (rc != DCA_E_BADARG || strncmp(msg, "bad argument: ", 14) != 0 || !strstr(msg, who) || !strstr(msg, word)) {
        printf("FAILED: %s / %s: rc %d, message %s\n", who, word, rc, msg);
        failures++;
    }
}

// next[i] = cur[perm[a][i]] (include/dca.h)
static void turn(uint8_t* state, int a) {
    const uint8_t* perm = dca_cube3_perm_table() + a * 54;
    uint8_t next[54];
    for (int i = 0; i < 54; i++) next[i] = state[perm[i]];
    memcpy(state, next, 54);
}

// the tiny set: corners {0, 1} and edges {0, 1}, each table of exactly its pattern's bytes, all zero
struct Tiny {
    const int kinds[2] = {DCA_CUBE3_CORNERS, DCA_CUBE3_EDGES}, ks[2] = {2, 2};
    const uint8_t cubies[4] = {0, 1, 0, 1};
    std::vector<uint8_t> corner = std::vector<uint8_t>(504, 0), edge = std::vector<uint8_t>(528, 0);
    const uint8_t* tables[2] = {corner.data(), edge.data()};
};

using Eval = int (*)(const uint8_t*, int64_t, int64_t, int, int, const int*, const uint8_t*, const int*, const uint8_t* const*, int, float*);
using Search = int (*)(const uint8_t*, int, const int*, const uint8_t*, const int*, const uint8_t* const*, int, int64_t, int*, int*, uint8_t*, int, int*,
                       int*, int64_t*, int, int64_t*);

static int64_t eval_cases(const Tiny& t) {
    if ((int64_t)t.corner.size() != dca_cube3_pdb_bytes(DCA_CUBE3_CORNERS, 2) || (int64_t)t.edge.size() != dca_cube3_pdb_bytes(DCA_CUBE3_EDGES, 2))
        fail("table sizes");
    int64_t rows_done = 0;
    const Eval evals[2] = {dca_cube3_pdb_eval_sym_host, dca_cube3_pdb_eval_dual_host};
    for (int ld : {54, 57})
        for (int row_kind : {DCA_ROWS_STATE, DCA_ROWS_NNET})
            for (int arbitrary = 0; arbitrary < 2; arbitrary++) {
                const int64_t n = 5;
                std::vector<uint8_t> rows((size_t)((n - 1) * ld + 54));  // exact size: the last row ends where the block ends
                for (auto& b : rows) b = (uint8_t)rnd();
                if (!arbitrary) {  // cube states: random walks from the goal, as sticker ids or as their colours
                    uint8_t s[54];
                    for (int i = 0; i < 54; i++) s[i] = (uint8_t)i;
                    for (int64_t r = 0; r < n; r++) {
                        for (int m = 0; m < 7; m++) turn(s, (int)(rnd() % 12));
                        for (int i = 0; i < 54; i++) rows[(size_t)(r * ld + i)] = row_kind == DCA_ROWS_STATE ? s[i] : (uint8_t)(s[i] / 9);
                    }
                }
                for (int which = 0; which < 2; which++)
                    for (int images : {1, 2, 48}) {
                        std::vector<float> out((size_t)n, -1.0f);
                        if (evals[which](rows.data(), n, ld, row_kind, 2, t.kinds, t.cubies, t.ks, t.tables, images, out.data()) != 0)
                            fail(dca_last_error(), which, images);
                        for (int64_t i = 0; i < n; i++)
                            if (out[(size_t)i] != 0.0f) fail("row value", which, i);  // every table byte is 0
                        rows_done += n;
                    }
            }
    return rows_done;
}

struct Found {
    int status = -1, length = -1, count = 0;
    int thresholds[8] = {};
    int64_t per[8] = {}, total = 0;
    uint8_t moves[8] = {};
};

static void check_found(const char* who, int rc, const Found& f, const uint8_t* root, int images) {
    if (rc != 0 || f.status != DCA_IDASTAR_SOLVED || f.length != 2 || f.count != 3 || f.thresholds[2] != 2 || f.total <= 0 || f.total > 100000) {
        fail(who, rc, images);
        return;
    }
    uint8_t s[54];
    memcpy(s, root, 54);
    for (int m = 0; m < f.length; m++) turn(s, f.moves[m]);
    for (int i = 0; i < 54; i++)
        if (s[i] != i) {
            fail("replay", images, i);
            return;
        }
}

static int search_cases(const Tiny& t) {
    std::vector<uint8_t> root(54);  // exact size
    for (int i = 0; i < 54; i++) root[(size_t)i] = (uint8_t)i;
    turn(root.data(), 0);
    turn(root.data(), 5);  // another face's quarter turn: no single move undoes the two
    int searches = 0;
    Found f;
    int rc = dca_idastar_host(DCA_ENV_CUBE3, 0, root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 100000, &f.status, &f.length, f.moves, 8, &f.count,
                              f.thresholds, f.per, 8, &f.total);
    check_found("dca_idastar_host", rc, f, root.data(), 0);
    searches++;
    const Search fns[2] = {dca_idastar_host_sym, dca_idastar_host_dual};
    const char* names[2] = {"dca_idastar_host_sym", "dca_idastar_host_dual"};
    for (int which = 0; which < 2; which++)
        for (int images : {1, 2, 48}) {
            Found g;
            rc = fns[which](root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, images, 100000, &g.status, &g.length, g.moves, 8, &g.count, g.thresholds, g.per,
                            8, &g.total);
            check_found(names[which], rc, g, root.data(), images);
            searches++;
        }
    return searches;
}

static void refusal_cases(const Tiny& t) {
    std::vector<uint8_t> rows(2 * 54, 0), root(54);
    for (int i = 0; i < 54; i++) root[(size_t)i] = (uint8_t)i;
    std::vector<uint8_t> twice = root;
    twice[53] = 0;
    std::vector<float> out(2, -3.0f);
    const uint8_t far[4] = {0, 1, 0, 12}, same[4] = {0, 0, 0, 1};
    const int odd_kinds[2] = {DCA_CUBE3_CORNERS, 2}, big_ks[2] = {2, 9};
    const uint8_t* with_null[2] = {t.corner.data(), nullptr};

    const Eval evals[2] = {dca_cube3_pdb_eval_sym_host, dca_cube3_pdb_eval_dual_host};
    const char* eval_names[2] = {"dca_cube3_pdb_eval_sym_host", "dca_cube3_pdb_eval_dual_host"};
    for (int which = 0; which < 2; which++) {
        const Eval e = evals[which];
        const char* E = eval_names[which];
        refused(e(rows.data(), -1, 54, 0, 2, t.kinds, t.cubies, t.ks, t.tables, 1, out.data()), E, "n >= 0");
        refused(e(rows.data(), 2, 53, 0, 2, t.kinds, t.cubies, t.ks, t.tables, 1, out.data()), E, "ld >= 54");
        refused(e(rows.data(), 2, 54, 2, 2, t.kinds, t.cubies, t.ks, t.tables, 1, out.data()), E, "row_kind");
        refused(e(rows.data(), 2, 54, 0, 0, t.kinds, t.cubies, t.ks, t.tables, 1, out.data()), E, "num_patterns = 0");
        refused(e(rows.data(), 2, 54, 0, 25, t.kinds, t.cubies, t.ks, t.tables, 1, out.data()), E, "num_patterns = 25");
        refused(e(rows.data(), 2, 54, 0, 2, nullptr, t.cubies, t.ks, t.tables, 1, out.data()), E, "must not be NULL");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, nullptr, t.ks, t.tables, 1, out.data()), E, "must not be NULL");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, t.cubies, nullptr, t.tables, 1, out.data()), E, "must not be NULL");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, t.cubies, t.ks, nullptr, 1, out.data()), E, "must not be NULL");
        refused(e(rows.data(), 2, 54, 0, 2, odd_kinds, t.cubies, t.ks, t.tables, 1, out.data()), E, "kind = 2");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, t.cubies, big_ks, t.tables, 1, out.data()), E, "k = 9");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, far, t.ks, t.tables, 1, out.data()), E, "cubie 12");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, same, t.ks, t.tables, 1, out.data()), E, "appears twice");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, t.cubies, t.ks, with_null, 1, out.data()), E, "table 1 is NULL");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, t.cubies, t.ks, t.tables, 0, out.data()), E, "max_images = 0");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, t.cubies, t.ks, t.tables, 49, out.data()), E, "max_images = 49");
        refused(e(nullptr, 2, 54, 0, 2, t.kinds, t.cubies, t.ks, t.tables, 1, out.data()), E, "states");
        refused(e(rows.data(), 2, 54, 0, 2, t.kinds, t.cubies, t.ks, t.tables, 1, nullptr), E, "out");
        if (e(nullptr, 0, 54, 0, 2, t.kinds, t.cubies, t.ks, t.tables, 1, nullptr) != 0) fail("n == 0", which);
    }
    if (out[0] != -3.0f || out[1] != -3.0f) fail("a refusal wrote");

    Found f;
    auto plain = [&](int env, const uint8_t* r, int np, const int* kinds, const uint8_t* ids, const int* ks, const uint8_t* const* tb, int64_t max_nodes,
                     int* status) {
        return dca_idastar_host(env, 0, r, np, kinds, ids, ks, tb, max_nodes, status, &f.length, f.moves, 8, &f.count, f.thresholds, f.per, 8, &f.total);
    };
    const char* H = "dca_idastar_host";
    refused(plain(7, root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 1000, &f.status), H, "env = 7");
    refused(plain(DCA_ENV_CUBE3, nullptr, 2, t.kinds, t.cubies, t.ks, t.tables, 1000, &f.status), H, "must not be NULL");
    refused(plain(DCA_ENV_CUBE3, root.data(), 2, nullptr, t.cubies, t.ks, t.tables, 1000, &f.status), H, "must not be NULL");
    refused(plain(DCA_ENV_CUBE3, root.data(), 0, t.kinds, t.cubies, t.ks, t.tables, 1000, &f.status), H, "num_patterns = 0");
    refused(plain(DCA_ENV_CUBE3, root.data(), 25, t.kinds, t.cubies, t.ks, t.tables, 1000, &f.status), H, "num_patterns = 25");
    refused(plain(DCA_ENV_CUBE3, root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 0, &f.status), H, "max_nodes");
    refused(plain(DCA_ENV_CUBE3, root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 1000, nullptr), H, "must not be NULL");
    refused(plain(DCA_ENV_CUBE3, root.data(), 2, odd_kinds, t.cubies, t.ks, t.tables, 1000, &f.status), H, "kind = 2");
    refused(plain(DCA_ENV_CUBE3, root.data(), 2, t.kinds, far, t.ks, t.tables, 1000, &f.status), H, "cubie 12");
    refused(plain(DCA_ENV_CUBE3, root.data(), 2, t.kinds, t.cubies, t.ks, with_null, 1000, &f.status), H, "table 1 is NULL");
    refused(plain(DCA_ENV_CUBE3, twice.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 1000, &f.status), H, "sticker ids");

    const Search fns[2] = {dca_idastar_host_sym, dca_idastar_host_dual};
    const char* names[2] = {"dca_idastar_host_sym", "dca_idastar_host_dual"};
    for (int which = 0; which < 2; which++) {
        const char* S = names[which];
        auto listed = [&](const uint8_t* r, int np, const int* kinds, const uint8_t* ids, const int* ks, const uint8_t* const* tb, int images,
                          int64_t max_nodes, int* status) {
            return fns[which](r, np, kinds, ids, ks, tb, images, max_nodes, status, &f.length, f.moves, 8, &f.count, f.thresholds, f.per, 8, &f.total);
        };
        refused(listed(nullptr, 2, t.kinds, t.cubies, t.ks, t.tables, 1, 1000, &f.status), S, "root must not be NULL");
        refused(listed(root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 1, 0, &f.status), S, "max_nodes");
        refused(listed(root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 1, 1000, nullptr), S, "must not be NULL");
        refused(listed(root.data(), 0, t.kinds, t.cubies, t.ks, t.tables, 1, 1000, &f.status), S, "num_patterns = 0");
        refused(listed(root.data(), 2, t.kinds, t.cubies, nullptr, t.tables, 1, 1000, &f.status), S, "must not be NULL");
        refused(listed(root.data(), 2, t.kinds, same, t.ks, t.tables, 1, 1000, &f.status), S, "appears twice");
        refused(listed(root.data(), 2, t.kinds, t.cubies, t.ks, with_null, 1, 1000, &f.status), S, "table 1 is NULL");
        refused(listed(root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 0, 1000, &f.status), S, "max_images = 0");
        refused(listed(root.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 49, 1000, &f.status), S, "max_images = 49");
        refused(listed(twice.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 1, 1000, &f.status), S, "sticker ids");
    }
    // 54 distinct ids that are no cube state (tests/test_cube3_dual_cpu.py's): two corner cubies are nowhere, and the colour rule
    // puts both at location 0.  The dual search alone names such a root.
    std::vector<uint8_t> mixed = root;
    mixed[0] = 10, mixed[10] = 0, mixed[8] = 12, mixed[12] = 8;
    refused(dca_idastar_host_dual(mixed.data(), 2, t.kinds, t.cubies, t.ks, t.tables, 1, 1000, &f.status, &f.length, f.moves, 8, &f.count, f.thresholds,
                                  f.per, 8, &f.total),
            "dca_idastar_host_dual", "no cube state");
}

int main() {
    const Tiny t;
    const int64_t rows = eval_cases(t);
    const int searches = search_cases(t);
    refusal_cases(t);
    printf("%lld rows, %d searches, %d refusals: %s\n", (long long)rows, searches, refusals, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
