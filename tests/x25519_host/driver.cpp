// Stand-alone host driver of rustyguard_amd/csrc/rg_x25519.h for tests/test_x25519_cpu.py: compiled with g++
// under AddressSanitizer and UBSan and run as a program.  It reads one command per line from stdin and
// answers each with one line of hex on stdout; the test states the expected values with Python integers.
//
//   x <k> <u>             X25519(k, u): 64 hex digits each -> "<out> <0|1>" (1 = the result is not all zero)
//   iter <n>              RFC 7748 §5.2's iteration from k = u = 9, n steps -> k
//   mul <m> <a> <b> <c> <d>   fe_mul(X, Y): m = two letters, X from (a, b) and Y from (c, d), each n (the first
//                         operand alone), s (the unreduced sum) or d (the unreduced difference)
//   sq|inv|a24 <m> <a> <b>    fe_sq / fe_invert / fe_mul121665 of X from (a, b), m = one letter as above
// Field operands go through fe_from_bytes, results through fe_to_bytes (canonical).  fe_invert takes a
// carried value, as in the ladder, so its sum / difference forms are carried by a multiplication by one first.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rg_x25519.h"

namespace {

bool unhex(const char *s, uint8_t out[32]) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 32; ++i) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

void put(const uint8_t b[32]) {
    for (int i = 0; i < 32; ++i) printf("%02x", b[i]);
}

uint32_t x25519(const uint8_t k[32], const uint8_t u[32], uint8_t out[32]) {
    uint32_t kw[8], uw[8], ow[8];
    rg::fe_words_from_bytes(k, kw);
    rg::fe_words_from_bytes(u, uw);
    const uint32_t nz = rg::x25519_words(kw, uw, ow);
    rg::fe_words_to_bytes(ow, out);
    return nz;
}

bool operand(char mode, const char *a, const char *b, rg::Fe *out) {
    uint8_t ab[32], bb[32];
    if (!unhex(a, ab) || !unhex(b, bb)) return false;
    const rg::Fe x = rg::fe_from_bytes(ab), y = rg::fe_from_bytes(bb);
    if (mode == 'n') *out = x;
    else if (mode == 's') *out = rg::fe_add(x, y);
    else if (mode == 'd') *out = rg::fe_sub(x, y);
    else return false;
    return true;
}

} // namespace

int main() {
    char line[512], op[8], m[80], a[80], b[80], c[80], d[80];
    while (fgets(line, sizeof line, stdin)) {
        uint8_t o[32];
        const int nf = sscanf(line, "%7s %79s %79s %79s %79s %79s", op, m, a, b, c, d);
        if (nf < 2) continue;
        const std::string cmd = op;
        if (cmd == "x" && nf == 3) {
            uint8_t k[32], u[32];
            if (!unhex(m, k) || !unhex(a, u)) return 2;
            const uint32_t nz = x25519(k, u, o);
            put(o);
            printf(" %d\n", nz != 0);
        } else if (cmd == "iter" && nf == 2) {
            uint8_t k[32] = {9}, u[32] = {9};
            const long n = atol(m);
            for (long i = 0; i < n; ++i) {
                x25519(k, u, o);
                memcpy(u, k, 32);
                memcpy(k, o, 32);
            }
            put(k);
            printf("\n");
        } else if (cmd == "mul" && nf == 6 && strlen(m) == 2) {
            rg::Fe x, y;
            if (!operand(m[0], a, b, &x) || !operand(m[1], c, d, &y)) return 2;
            rg::fe_to_bytes(rg::fe_mul(x, y), o);
            put(o);
            printf("\n");
        } else if ((cmd == "sq" || cmd == "inv" || cmd == "a24") && nf == 4 && strlen(m) == 1) {
            rg::Fe x;
            if (!operand(m[0], a, b, &x)) return 2;
            if (cmd == "inv" && m[0] != 'n') x = rg::fe_mul(x, rg::fe_small(1));
            const rg::Fe r = cmd == "sq" ? rg::fe_sq(x) : cmd == "inv" ? rg::fe_invert(x) : rg::fe_mul121665(x);
            rg::fe_to_bytes(r, o);
            put(o);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
