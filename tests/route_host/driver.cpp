// Stand-alone host driver of rustyguard_amd/csrc/rg_route.h for tests/test_route_cpu.py: compiled with g++ under
// AddressSanitizer and UBSan and run as a program.  It reads commands from stdin and answers each with one line
// on stdout; the test states the expected values with a brute-force longest-prefix match in Python.
//
//   t <np>  then np lines "<addr hex8> <prefix_len> <peer>"
//           builds the table into a heap buffer of exactly rg::route::table_words words (a one-word overrun is
//           a sanitizer report), a second time into another buffer (determinism), and once into a buffer one
//           word short           -> "<words> <rc> <same 0|1> <rc one word short>"
//   p <k>   then k lines "<addr hex8>": looks each up in the last table -> k results in hex, space separated
//   c       corrupt tables: pointers to blocks at and past the end of the table, on the root, on the second
//           level and (a pointer where only leaves may stand) on the third; every lookup must come back
//           RG_PEER_NONE without reading outside the exactly sized buffer -> "<lookups> <results that were not NONE>"
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "rg_route.h"

namespace {

uint32_t lookup(const std::vector<uint32_t> &t, uint32_t a) {
    const uint8_t b[4] = {(uint8_t)(a >> 24), (uint8_t)(a >> 16), (uint8_t)(a >> 8), (uint8_t)a};
    return rg::route::lookup(t.data(), t.size(), rg::route::addr_be(b));
}

int corrupt() {
    using namespace rg::route;
    unsigned lookups = 0, bad = 0;
    const uint32_t probes[] = {0u, 0x0A010203u, 0x0A0102FFu, 0x0A01FF03u, 0xFFFFFFFFu, 0x7F000001u, 0x0A010000u};
    // (words of the table, pointer planted) -- block numbers at the end, one past it, far past it, the largest
    for (uint32_t blocks = 0; blocks <= 2; ++blocks) {
        const uint32_t ptrs[] = {kPointer | blocks, kPointer | (blocks + 1), kPointer | 0x00FFFFFFu, kPointer | 0x7FFFFFFEu};
        for (uint32_t ptr : ptrs) {
            for (int level = 0; level < 3; ++level) {
                if ((uint32_t)level > blocks) continue;
                // exactly sized, on the heap: a read one word past it is a sanitizer report
                std::vector<uint32_t> t((size_t)kRootWords + (size_t)kBlockWords * blocks, 7u);
                t.shrink_to_fit();
                if (level == 0) {
                    std::fill(t.begin(), t.begin() + kRootWords, ptr);
                } else if (level == 1) { // root -> block 0 (valid), whose entries point past the end
                    std::fill(t.begin(), t.begin() + kRootWords, kPointer | 0u);
                    std::fill(t.begin() + kRootWords, t.begin() + kRootWords + kBlockWords, ptr);
                } else { // root -> block 0 -> block 1 (both valid), whose entries are pointers: not allowed there
                    std::fill(t.begin(), t.begin() + kRootWords, kPointer | 0u);
                    std::fill(t.begin() + kRootWords, t.begin() + kRootWords + kBlockWords, kPointer | 1u);
                    std::fill(t.begin() + kRootWords + kBlockWords, t.end(), ptr);
                }
                for (uint32_t a : probes) {
                    ++lookups;
                    if (lookup(t, a) != RG_PEER_NONE) ++bad;
                }
            }
        }
    }
    printf("%u %u\n", lookups, bad);
    return 0;
}

} // namespace

int main() {
    std::vector<uint32_t> table;
    char cmd[8];
    unsigned k;
    while (scanf("%7s", cmd) == 1) {
        if (!strcmp(cmd, "c")) {
            corrupt();
        } else if (!strcmp(cmd, "t") && scanf("%u", &k) == 1) {
            std::vector<rg_route_prefix> rows(k);
            for (auto &r : rows) {
                unsigned a, len, peer;
                if (scanf("%x %u %u", &a, &len, &peer) != 3) return 2;
                r = rg_route_prefix{{(uint8_t)(a >> 24), (uint8_t)(a >> 16), (uint8_t)(a >> 8), (uint8_t)a}, len, peer};
            }
            const rg_route_prefix *p = rows.empty() ? nullptr : rows.data();
            const size_t words = rg::route::table_words(p, k);
            // new[]: exactly `words` words, no slack behind them
            std::unique_ptr<uint32_t[]> a(new uint32_t[words ? words : 1]), b(new uint32_t[words ? words : 1]);
            std::unique_ptr<uint32_t[]> s(new uint32_t[words > 1 ? words - 1 : 1]);
            const int rc = rg::route::table_build(p, k, a.get(), words);
            const int rc2 = rg::route::table_build(p, k, b.get(), words);
            const int rc_short = rg::route::table_build(p, k, s.get(), words ? words - 1 : 0);
            const bool same = rc == RG_OK && rc2 == RG_OK && !memcmp(a.get(), b.get(), words * sizeof(uint32_t));
            table.assign(a.get(), a.get() + (rc == RG_OK ? words : 0));
            table.shrink_to_fit();
            printf("%zu %d %d %d\n", words, rc, same ? 1 : 0, rc_short);
        } else if (!strcmp(cmd, "p") && scanf("%u", &k) == 1) {
            for (unsigned i = 0; i < k; ++i) {
                unsigned a;
                if (scanf("%x", &a) != 1) return 2;
                const uint32_t r = table.size() >= rg::route::kRootWords ? lookup(table, a) : RG_PEER_NONE;
                printf("%x%c", r, i + 1 == k ? '\n' : ' ');
            }
            if (k == 0) printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
