// The pattern-database entry points' host code under AddressSanitizer / UBSan, on a CPU (no device is touched): every refusal
// that returns before the first HIP call — the cases of tests/test_pdb_cpu.py and tests/test_cube3_pdb_cpu.py — and
// dca_cube3_pdb_index on a few rows.  A stand-alone program, so the sanitizer's runtime is linked in, not preloaded:
//
//   cd deepcubea_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I ../../include ../../tools/pdb_refusals_asan.cpp dca_pdb.hip dca_pdb_cube3.hip dca_env.hip -o /tmp/pdb_refusals_asan
//   /tmp/pdb_refusals_asan        # prints "N refusals, M indices: ok", exit status 0; a sanitizer report otherwise
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <utility>
#include <vector>

#include "dca.h"

static int refusals = 0, failures = 0;

static void refused(long long rc, const char* who, const char* word) {
    const char* msg = dca_last_error();
    refusals++;
    if (rc != DCA_E_BADARG || strncmp(msg, "bad argument: ", 14) != 0 || !strstr(msg, who) || !strstr(msg, word)) {
        printf("FAILED: %s / %s: rc %lld, message %s\n", who, word, rc, msg);
        failures++;
    }
}

using Ids = std::vector<uint8_t>;
using Groups = std::vector<Ids>;
static uint8_t* const one = (uint8_t*)64;  // never dereferenced: every call that takes it is refused

static int p_build(int dim, Ids t, int k = -1, uint8_t* table = one) {
    return dca_pdb_build(dim, t.data(), k < 0 ? (int)t.size() : k, table, nullptr, nullptr);
}

// exact-size arrays, as a caller's numpy arrays are: a read past an id list or a ks list is a heap overflow here
static int p_eval(Groups g, int dim = 4, int64_t n = 8, int64_t ld = 16, const uint8_t* states = one, float* out = (float*)one,
                  int np = -1, int null_at = -1, const std::vector<int>* kinds = nullptr, int row_kind = 0) {
    Ids flat;
    std::vector<int> ks;
    for (auto& x : g) {
        flat.insert(flat.end(), x.begin(), x.end());
        ks.push_back((int)x.size());
    }
    std::vector<const uint8_t*> tables(g.size() ? g.size() : 1, one);
    if (null_at >= 0) tables[null_at] = nullptr;
    const int m = np < 0 ? (int)g.size() : np;
    if (kinds) return dca_cube3_pdb_eval(states, n, ld, row_kind, m, kinds->data(), flat.data(), ks.data(), tables.data(), out, nullptr);
    return dca_pdb_eval(dim, states, n, ld, m, flat.data(), ks.data(), tables.data(), out, nullptr);
}

static int c_eval(std::vector<int> kinds, Groups g, int64_t n = 8, int64_t ld = 54, const uint8_t* states = one, float* out = (float*)one,
                  int np = -1, int null_at = -1, int row_kind = 1) {
    return p_eval(g, 0, n, ld, states, out, np, null_at, &kinds, row_kind);
}

static int c_build(int kind, Ids c, int k = -1, uint8_t* table = one) {
    return dca_cube3_pdb_build(kind, c.data(), k < 0 ? (int)c.size() : k, table, nullptr, nullptr);
}

static int c_index(int kind, Ids c, const uint8_t* row, int row_kind, int64_t* index, int k = -1) {
    return dca_cube3_pdb_index(kind, c.data(), k < 0 ? (int)c.size() : k, row, row_kind, index);
}

int main() {
    const char *B = "dca_pdb_build", *E = "dca_pdb_eval", *CB = "dca_cube3_pdb_build", *CE = "dca_cube3_pdb_eval", *CI = "dca_cube3_pdb_index";
    for (auto dk : {std::pair<int, int>{2, 1}, {8, 1}, {3, 0}, {3, 9}, {4, 8}, {7, 6}}) refused(dca_pdb_bytes(dk.first, dk.second), "dca_pdb_bytes", "");
    for (auto kk : {std::pair<int, int>{2, 1}, {-1, 1}, {0, 0}, {0, 9}, {1, -1}}) refused(dca_cube3_pdb_bytes(kk.first, kk.second), "dca_cube3_pdb_bytes", "");
    uint8_t pos[24];
    refused(dca_cube3_pdb_cubies(2, pos), "dca_cube3_pdb_cubies", "kind");
    refused(dca_cube3_pdb_cubies(0, nullptr), "dca_cube3_pdb_cubies", "positions");

    refused(p_build(4, {1, 2, 3}, 0), B, "k = 0");
    refused(p_build(4, {0, 1}), B, "tile 0");
    refused(p_build(4, {1, 16}), B, "tile 16");
    refused(p_build(4, {1, 2, 1}), B, "tile 1 appears twice");
    refused(p_build(4, {1, 2, 3}, -1, nullptr), B, "table");
    refused(p_build(2, {1}), B, "dim");
    refused(p_build(8, {1}), B, "dim");
    refused(p_build(4, {1, 2, 3, 4, 5, 6, 7, 8}), B, "2^34");
    refused(dca_pdb_build(4, nullptr, 3, one, nullptr, nullptr), B, "tiles");

    refused(p_eval({{1, 2}, {}}), E, "k = 0");
    refused(p_eval({{0, 2}}), E, "tile 0");
    refused(p_eval({{1, 16}}), E, "tile 16");
    refused(p_eval({{1, 2, 3}, {4, 2}}), E, "tile 2 appears twice");
    Groups ones;
    for (int t = 1; t <= 25; t++) ones.push_back({(uint8_t)t});
    refused(p_eval(ones, 7, 8, 49), E, "num_patterns");
    refused(p_eval({}, 4, 8, 16, one, (float*)one, 0), E, "num_patterns");
    refused(p_eval({{1, 2, 3}, {4, 5}}, 4, 8, 16, one, (float*)one, -1, 1), E, "table 1 is NULL");
    refused(p_eval({{1, 2, 3}}, 4, 8, 15), E, "ld");
    refused(p_eval({{1, 2, 3}}, 5, 8, 24), E, "ld");
    refused(p_eval({{1, 2, 3}}, 2), E, "dim");
    refused(p_eval({{1, 2, 3}}, 8), E, "dim");
    refused(p_eval({{1, 2, 3}}, 4, -1), E, "n >= 0");
    refused(p_eval({{1, 2, 3}}, 4, (int64_t)1 << 31), E, "n >= 0");
    refused(p_eval({{1, 2, 3}}, 4, 8, 16, nullptr), E, "states");
    refused(p_eval({{1, 2, 3}}, 4, 8, 16, one, nullptr), E, "out");
    refused(p_eval({{1, 2, 3}}, 4, 8, 16, one, (float*)66), E, "out");
    if (p_eval({{1, 2, 3}, {4, 5}}, 4, 0, 16, nullptr, nullptr) != 0) failures++;  // n == 0: nothing to do, nothing launched

    refused(c_build(2, {0}), CB, "kind");
    refused(c_build(0, {0, 1}, 0), CB, "k = 0");
    refused(c_build(0, {0, 0, 0, 0, 0, 0, 0, 0, 0}), CB, "k = 9");
    refused(c_build(0, {0, 8}), CB, "cubie 8");
    refused(c_build(1, {12}), CB, "cubie 12");
    refused(c_build(1, {3, 1, 3}), CB, "cubie 3 appears twice");
    refused(c_build(0, {0, 1}, -1, nullptr), CB, "table");
    refused(dca_cube3_pdb_build(0, nullptr, 2, one, nullptr, nullptr), CB, "cubies");

    refused(c_eval({0, 2}, {{0, 1}, {2}}), CE, "kind");
    refused(c_eval({0, 1}, {{0, 1}, {}}), CE, "k = 0");
    refused(c_eval({1}, {{0, 1, 2, 3, 4, 5, 6, 7, 8}}), CE, "k = 9");
    refused(c_eval({0}, {{0, 8}}), CE, "cubie 8");
    refused(c_eval({0, 1}, {{0, 1}, {4, 4}}), CE, "cubie 4 appears twice");
    refused(c_eval(std::vector<int>(25, 1), Groups(25, Ids{0})), CE, "num_patterns");
    refused(c_eval({}, {}, 8, 54, one, (float*)one, 0), CE, "num_patterns");
    refused(c_eval({0, 1}, {{0, 1}, {2}}, 8, 54, one, (float*)one, -1, 0), CE, "table 0 is NULL");
    refused(c_eval({0}, {{0}}, 8, 53), CE, "ld");
    refused(c_eval({0}, {{0}}, -1), CE, "n >= 0");
    refused(c_eval({0}, {{0}}, 8, 54, one, (float*)one, -1, -1, 2), CE, "row_kind");
    refused(c_eval({0}, {{0}}, 8, 54, nullptr), CE, "states");
    refused(c_eval({0}, {{0}}, 8, 54, one, nullptr), CE, "out");
    if (c_eval({0, 1}, {{0, 1}, {2}}, 0, 54, nullptr, nullptr) != 0) failures++;

    uint8_t row[54];
    for (int i = 0; i < 54; i++) row[i] = (uint8_t)i;
    int64_t index = -7;
    refused(c_index(2, {0, 1}, row, 0, &index), CI, "kind");
    refused(c_index(0, {0, 1}, row, 0, &index, 0), CI, "k = 0");
    refused(c_index(0, {0, 8}, row, 0, &index), CI, "cubie 8");
    refused(c_index(0, {3, 1, 3}, row, 0, &index), CI, "cubie 3 appears twice");
    refused(c_index(0, {0, 1}, nullptr, 0, &index), CI, "row");
    refused(c_index(0, {0, 1}, row, 2, &index), CI, "row_kind");
    refused(c_index(0, {0, 1}, row, 0, nullptr), CI, "index");
    if (index != -7) failures++;

    // the index of a few rows, each an exact 54-byte heap block: the goal, its colours, all 0xFF, a byte ramp
    int indices = 0;
    for (int which = 0; which < 4; which++) {
        std::vector<uint8_t> r(54);
        for (int i = 0; i < 54; i++) r[i] = which == 0 ? (uint8_t)i : which == 1 ? (uint8_t)(i / 9) : which == 2 ? 0xFF : (uint8_t)(5 * i);
        for (int kind = 0; kind < 2; kind++)
            for (Ids c : {Ids{0}, Ids{7, 3, 0}, Ids{0, 1, 2, 3, 4, 5, 6, 7}}) {
                const int64_t total = dca_cube3_pdb_bytes(kind, (int)c.size());
                if (c_index(kind, c, r.data(), which == 1, &index) != 0 || index < 0 || index >= total) failures++;
                indices++;
            }
    }
    if (c_index(1, {11}, row, 0, &index) != 0 || index != 22) failures++;
    printf("%d refusals, %d indices: %s\n", refusals, indices, failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
