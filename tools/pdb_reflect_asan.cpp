// The reflected look-up's host code under AddressSanitizer / UBSan, on a CPU (no device is touched, no Python): the kernels' own
// row value through dca_pdb_eval_host — plain and reflected, rows of random bytes (all 256 values) on exact-size heap tables, so
// an index past a table or a row is a heap overflow here — the kernel's search code through dca_idastar_host_reflected on a few
// puzzle8 roots, and the new refusals.  A stand-alone program, so the sanitizer's runtime is linked in, not preloaded:
//
//   cd deepcubea_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I ../../include ../../tools/pdb_reflect_asan.cpp dca_pdb.hip dca_idastar.hip dca_pdb_cube3.hip dca_env.hip -o /tmp/pdb_reflect_asan
//   /tmp/pdb_reflect_asan        # prints "N rows, M searches, K refusals: ok", exit status 0; a sanitizer report otherwise
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
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

static int refl(int dim, int p) { return (p % dim) * dim + p / dim; }
static int phi(int dim, int t) { return t == 0 ? 0 : refl(dim, t - 1) + 1; }

// the any-bytes rule: the last position < N that holds t, 0 if none
static int pos_of(const uint8_t* row, int N, int t) {
    int p = 0;
    for (int i = 0; i < N; i++)
        if (row[i] == t) p = i;
    return p;
}

// include/dca.h's definition, restated: the plain sum, or the larger of it and the sum at the reflected indices
static uint32_t value(int dim, const uint8_t* row, const std::vector<std::vector<uint8_t>>& groups, const std::vector<std::vector<uint8_t>>& tables,
                      bool reflect) {
    const int N = dim * dim;
    uint32_t sum = 0, rsum = 0;
    for (size_t g = 0; g < groups.size(); g++) {
        uint64_t idx = 0, ridx = 0;
        for (int j = (int)groups[g].size() - 1; j >= 0; j--) {
            idx = idx * N + pos_of(row, N, groups[g][j]);
            ridx = ridx * N + refl(dim, pos_of(row, N, phi(dim, groups[g][j])));
        }
        sum += tables[g][idx * N + pos_of(row, N, 0)];
        rsum += tables[g][ridx * N + refl(dim, pos_of(row, N, 0))];
    }
    return reflect && rsum > sum ? rsum : sum;
}

static int64_t eval_cases() {
    int64_t rows_done = 0;
    for (int dim : {3, 4, 5, 7}) {
        const int N = dim * dim;
        const std::vector<std::vector<uint8_t>> groups = {{2, (uint8_t)(N - 1)}, {(uint8_t)(N - 2), 1}};
        std::vector<std::vector<uint8_t>> tables;
        for (size_t g = 0; g < groups.size(); g++) {
            tables.emplace_back((size_t)N * N * N);
            for (auto& b : tables.back()) b = (uint8_t)rnd();
        }
        const uint8_t tiles[4] = {groups[0][0], groups[0][1], groups[1][0], groups[1][1]};
        const int ks[2] = {2, 2};
        const uint8_t* ptrs[2] = {tables[0].data(), tables[1].data()};
        for (int ld : {N, N + 3})
            for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)257}) {
                std::vector<uint8_t> states((size_t)(n * ld));  // exact size: the last row ends where the block ends
                for (auto& b : states) b = (uint8_t)rnd();
                for (int reflect = 0; reflect < 2; reflect++) {
                    std::vector<float> out((size_t)n, -1.0f);
                    if (dca_pdb_eval_host(dim, states.data(), n, ld, 2, tiles, ks, ptrs, reflect, out.data()) != 0) fail("dca_pdb_eval_host", dim, ld);
                    for (int64_t i = 0; i < n; i++)
                        if (out[i] != (float)value(dim, states.data() + i * ld, groups, tables, reflect != 0)) fail("row value", dim, i);
                    rows_done += n;
                }
            }
    }
    return rows_done;
}

// one puzzle8 pattern's table by the header's cost rule: relaxation sweeps to the fixed point
static std::vector<uint8_t> p8_table(const std::vector<uint8_t>& tiles) {
    const int N = 9, k = (int)tiles.size();
    size_t total = N;
    for (int j = 0; j < k; j++) total *= N;
    std::vector<uint8_t> t(total, 0xFF);
    std::vector<int> d(k + 1);
    auto digits = [&](size_t e) {
        for (int j = 0; j <= k; j++, e /= N) d[j] = (int)(e % N);
    };
    for (size_t e = 0; e < total; e++) {
        digits(e);
        bool distinct = true, goal = d[0] == N - 1;
        for (int a = 0; a <= k; a++)
            for (int b = a + 1; b <= k; b++) distinct = distinct && d[a] != d[b];
        for (int j = 0; j < k; j++) goal = goal && d[j + 1] == tiles[j] - 1;
        if (distinct) t[e] = goal ? 0 : 0xFE;
    }
    for (bool changed = true; changed;) {
        changed = false;
        for (size_t e = 0; e < total; e++) {
            if (t[e] == 0xFF || t[e] == 0) continue;
            digits(e);
            const int z = d[0], zi = z / 3, zj = z % 3;
            const int nbs[4] = {zi < 2 ? z + 3 : z, zi > 0 ? z - 3 : z, zj < 2 ? z + 1 : z, zj > 0 ? z - 1 : z};
            for (int nb : nbs) {
                if (nb == z) continue;
                int64_t ne = (int64_t)e + nb - z, w = N;
                int cost = 0;
                for (int j = 1; j <= k; j++, w *= N)
                    if (d[j] == nb) {
                        ne += w * (z - nb);
                        cost = 1;
                    }
                if (t[(size_t)ne] < 0xFE && t[(size_t)ne] + cost < t[e]) {
                    t[e] = (uint8_t)(t[(size_t)ne] + cost);
                    changed = true;
                }
            }
        }
    }
    return t;
}

struct Search {
    int status = -1, length = -1, count = 0;
    int thresholds[64] = {};
    int64_t per[64] = {}, total = 0;
    uint8_t moves[64] = {};
};

static int search_cases(const std::vector<std::vector<uint8_t>>& tables) {
    const uint8_t tiles[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    const int ks[2] = {4, 4};
    const uint8_t* ptrs[2] = {tables[0].data(), tables[1].data()};
    int searches = 0;
    for (int walk : {0, 1, 7, 20, 45, 80}) {
        std::vector<uint8_t> root = {1, 2, 3, 4, 5, 6, 7, 8, 0};  // exact size
        int z = 8;
        for (int m = 0; m < walk; m++) {  // a random walk from the goal: always the goal's parity
            const int zi = z / 3, zj = z % 3;
            const int nbs[4] = {zi < 2 ? z + 3 : z, zi > 0 ? z - 3 : z, zj < 2 ? z + 1 : z, zj > 0 ? z - 1 : z};
            const int nb = nbs[rnd() & 3];
            root[z] = root[nb];
            root[nb] = 0;
            z = nb;
        }
        Search plain, mirrored;
        if (dca_idastar_host(DCA_ENV_NPUZZLE, 3, root.data(), 2, nullptr, tiles, ks, ptrs, (int64_t)1 << 40, &plain.status, &plain.length, plain.moves,
                             64, &plain.count, plain.thresholds, plain.per, 64, &plain.total) != 0)
            fail("dca_idastar_host", walk);
        if (dca_idastar_host_reflected(3, root.data(), 2, tiles, ks, ptrs, (int64_t)1 << 40, &mirrored.status, &mirrored.length, mirrored.moves, 64,
                                       &mirrored.count, mirrored.thresholds, mirrored.per, 64, &mirrored.total) != 0)
            fail("dca_idastar_host_reflected", walk);
        if (plain.status != DCA_IDASTAR_SOLVED || mirrored.status != DCA_IDASTAR_SOLVED || plain.length != mirrored.length || mirrored.length > walk)
            fail("lengths", plain.length, mirrored.length);
        std::vector<uint8_t> cur = root;
        for (int m = 0; m < mirrored.length && m < 64; m++) {
            const int b = (int)(std::find(cur.begin(), cur.end(), 0) - cur.begin()), bi = b / 3, bj = b % 3;
            const int nbs[4] = {bi < 2 ? b + 3 : b, bi > 0 ? b - 3 : b, bj < 2 ? b + 1 : b, bj > 0 ? b - 1 : b};
            const int nb = nbs[mirrored.moves[m] & 3];
            cur[b] = cur[nb];
            cur[nb] = 0;
        }
        if (cur != std::vector<uint8_t>{1, 2, 3, 4, 5, 6, 7, 8, 0}) fail("replay", walk);
        searches += 2;
    }
    return searches;
}

static void refusal_cases(const std::vector<std::vector<uint8_t>>& tables) {
    const char *H = "dca_idastar_host_reflected", *E = "dca_pdb_eval_host";
    const uint8_t tiles[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    const int ks[2] = {4, 4}, ones[5] = {1, 1, 1, 1, 1};
    const uint8_t* ptrs[5] = {tables[0].data(), tables[1].data(), tables[0].data(), tables[0].data(), tables[0].data()};
    const std::vector<uint8_t> good = {1, 2, 3, 4, 5, 6, 0, 7, 8}, odd = {2, 1, 3, 4, 5, 6, 0, 7, 8};
    Search s;
    auto host = [&](int dim, const uint8_t* root, int np, const uint8_t* t, const int* k, const uint8_t* const* tb, int64_t max_nodes, int* status) {
        return dca_idastar_host_reflected(dim, root, np, t, k, tb, max_nodes, status, &s.length, s.moves, 64, &s.count, s.thresholds, s.per, 64, &s.total);
    };
    refused(host(3, good.data(), 5, tiles, ones, ptrs, 1000, &s.status), H, "num_patterns = 5");
    refused(host(3, good.data(), 0, tiles, ks, ptrs, 1000, &s.status), H, "num_patterns");
    refused(host(3, nullptr, 2, tiles, ks, ptrs, 1000, &s.status), H, "NULL");
    refused(host(3, good.data(), 2, nullptr, ks, ptrs, 1000, &s.status), H, "NULL");
    refused(host(3, good.data(), 2, tiles, nullptr, ptrs, 1000, &s.status), H, "NULL");
    refused(host(3, good.data(), 2, tiles, ks, nullptr, 1000, &s.status), H, "NULL");
    refused(host(3, good.data(), 2, tiles, ks, ptrs, 1000, nullptr), H, "NULL");
    refused(host(3, good.data(), 2, tiles, ks, ptrs, 0, &s.status), H, "max_nodes");
    refused(host(3, odd.data(), 2, tiles, ks, ptrs, 1000, &s.status), H, "parity");
    refused(host(6, good.data(), 2, tiles, ks, ptrs, 1000, &s.status), H, "dim");
    refused(host(2, good.data(), 2, tiles, ks, ptrs, 1000, &s.status), H, "dim");

    std::vector<uint8_t> rows(8 * 9, 0);
    std::vector<float> out(8);
    const uint8_t twice[8] = {1, 2, 3, 4, 4, 6, 7, 8};
    const uint8_t* with_null[2] = {tables[0].data(), nullptr};
    refused(dca_pdb_eval_host(2, rows.data(), 8, 9, 2, tiles, ks, ptrs, 1, out.data()), E, "dim");
    refused(dca_pdb_eval_host(8, rows.data(), 8, 9, 2, tiles, ks, ptrs, 1, out.data()), E, "dim");
    refused(dca_pdb_eval_host(3, rows.data(), 8, 8, 2, tiles, ks, ptrs, 1, out.data()), E, "ld");
    refused(dca_pdb_eval_host(3, rows.data(), -1, 9, 2, tiles, ks, ptrs, 1, out.data()), E, "n >= 0");
    refused(dca_pdb_eval_host(3, rows.data(), 8, 9, 0, tiles, ks, ptrs, 1, out.data()), E, "num_patterns");
    refused(dca_pdb_eval_host(3, rows.data(), 8, 9, 25, tiles, ks, ptrs, 1, out.data()), E, "num_patterns");
    refused(dca_pdb_eval_host(3, rows.data(), 8, 9, 2, nullptr, ks, ptrs, 1, out.data()), E, "tiles");
    refused(dca_pdb_eval_host(3, rows.data(), 8, 9, 2, twice, ks, ptrs, 0, out.data()), E, "tile 4 appears twice");
    refused(dca_pdb_eval_host(3, rows.data(), 8, 9, 2, tiles, ks, with_null, 1, out.data()), E, "table 1 is NULL");
    refused(dca_pdb_eval_host(3, nullptr, 8, 9, 2, tiles, ks, ptrs, 1, out.data()), E, "states");
    refused(dca_pdb_eval_host(3, rows.data(), 8, 9, 2, tiles, ks, ptrs, 1, nullptr), E, "out");
    if (dca_pdb_eval_host(3, nullptr, 0, 9, 2, tiles, ks, ptrs, 1, nullptr) != 0) fail("n == 0");
    // the device entry point refuses before any HIP call, like dca_pdb_eval
    refused(dca_pdb_eval_reflected(3, rows.data(), 8, 8, 2, tiles, ks, ptrs, out.data(), nullptr), "dca_pdb_eval_reflected", "ld");
    refused(dca_idastar_npuzzle_reflected(3, good.data(), 5, tiles, ones, ptrs, 1000, &s.status, &s.length, s.moves, 64, &s.count, s.thresholds, s.per,
                                          64, &s.total, nullptr),
            "dca_idastar_npuzzle_reflected", "num_patterns = 5");
}

int main() {
    const int64_t rows = eval_cases();
    const std::vector<std::vector<uint8_t>> tables = {p8_table({1, 2, 3, 4}), p8_table({5, 6, 7, 8})};
    const int searches = search_cases(tables);
    refusal_cases(tables);
    printf("%lld rows, %d searches, %d refusals: %s\n", (long long)rows, searches, refusals, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
