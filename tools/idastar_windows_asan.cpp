// The bounded cube3 batch's host code under AddressSanitizer / UBSan, on a CPU (no device is touched, no Python):
// dca_idastar_host_cube3_batch — the batch driver, the rounds and the bound that dca_idastar_cube3_batch runs, with the
// sequential lane in place of the kernel — on five roots 0, 2 and 3 moves from the goal (one of them twice), plain, on 2 and 48
// images and on the dual look-ups, free and with a bound per root, on exact-size heap tables of zeros (one corner pattern of 2
// cubies, 504 bytes; one edge pattern of 2 cubies, 528 bytes) and exact-size output arrays, so an index past a table, a root
// or an output is a heap overflow here; then a refusal and a call without move and threshold buffers.  A stand-alone
// program, so the sanitizer's runtime is linked in, not preloaded:
//
//   cd deepcubea_amd/csrc && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I ../../include ../../tools/idastar_windows_asan.cpp dca_idastar.hip dca_pdb_cube3.hip dca_env.hip -o /tmp/idastar_windows_asan
//   /tmp/idastar_windows_asan      # prints "10 calls: ok", exit status 0; a sanitizer report otherwise
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "dca.h"
#include "dca_debug.h"
int main() {
    const uint8_t* perm = dca_cube3_perm_table();
    const int N = 5;
    std::vector<uint8_t> roots((size_t)N * 54);
    const int seqs[N][3] = {{0, 5, 7}, {2, 9, -1}, {-1, -1, -1}, {4, 4, 10}, {0, 5, 7}};
    for (int r = 0; r < N; r++) {
        uint8_t cur[54], nxt[54];
        for (int i = 0; i < 54; i++) cur[i] = (uint8_t)i;
        for (int j = 0; j < 3; j++) {
            if (seqs[r][j] < 0) continue;
            for (int i = 0; i < 54; i++) nxt[i] = cur[perm[seqs[r][j] * 54 + i]];
            memcpy(cur, nxt, 54);
        }
        memcpy(&roots[(size_t)r * 54], cur, 54);
    }
    std::vector<uint8_t> corner(504, 0), edge(528, 0);
    const int kinds[2] = {DCA_CUBE3_CORNERS, DCA_CUBE3_EDGES}, ks[2] = {2, 2};
    const uint8_t cubies[4] = {0, 1, 0, 1};
    const uint8_t* tables[2] = {corner.data(), edge.data()};
    int fails = 0, calls = 0;
    for (int mode = 0; mode < 4; mode++) {
        const int images = mode == 0 ? 0 : mode == 1 ? 2 : 48, dual = mode == 3;
        for (int bounded = 0; bounded < 2; bounded++) {
            const int cap = 6;  // exact-size outputs
            std::vector<int> status(N, -1), length(N, -1), count(N, -1), thr((size_t)N * cap, -1), bound = {1, 2, 0, 3, 254};
            std::vector<int64_t> per((size_t)N * cap, -1), total(N, -1);
            std::vector<uint8_t> moves((size_t)N * cap, 99);
            const int rc = dca_idastar_host_cube3_batch(roots.data(), N, 2, kinds, cubies, ks, tables, images, dual, bounded ? bound.data() : nullptr,
                                                        1000000, status.data(), length.data(), moves.data(), cap, count.data(), thr.data(),
                                                        per.data(), cap, total.data());
            calls++;
            if (rc != 0) { printf("FAILED rc %d: %s\n", rc, dca_last_error()); fails++; continue; }
            for (int r = 0; r < N; r++) {
                const int want = seqs[r][0] < 0 ? 0 : seqs[r][2] < 0 ? 2 : 3;
                const bool cut = bounded && want > bound[r];
                if (status[r] != (cut ? DCA_IDASTAR_BOUNDED : DCA_IDASTAR_SOLVED) || (!cut && length[r] != want)) {
                    printf("FAILED mode %d bounded %d root %d: status %d length %d\n", mode, bounded, r, status[r], length[r]);
                    fails++;
                }
            }
        }
    }
    std::vector<int> s(N), l(N), c(N); std::vector<int64_t> t(N);
    const int neg[N] = {1, 1, -2, 1, 1};
    int rc = dca_idastar_host_cube3_batch(roots.data(), N, 2, kinds, cubies, ks, tables, 0, 0, neg, 1000, s.data(), l.data(), nullptr, 0, c.data(), nullptr, nullptr, 0, t.data());
    if (rc != DCA_E_BADARG || !strstr(dca_last_error(), "max_length[2]")) { printf("FAILED refusal: %d %s\n", rc, dca_last_error()); fails++; }
    rc = dca_idastar_host_cube3_batch(roots.data(), N, 2, kinds, cubies, ks, tables, 0, 0, nullptr, 1000, s.data(), l.data(), nullptr, 0, c.data(), nullptr, nullptr, 0, t.data());
    if (rc != 0) { printf("FAILED no-capacity call: %d %s\n", rc, dca_last_error()); fails++; }
    printf("%d calls: %s\n", calls + 2, fails ? "FAILED" : "ok");
    return fails != 0;
}
