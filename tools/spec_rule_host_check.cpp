// Stand-alone front end of the integer rule of mm_spec_sample_rows (micromix_amd/csrc/mx_spec_rule.h: the 24-bit uniform number, mulshift,
// the accept predicate, a token's residual mass), so that the functions the kernels call are run against Python integers.  It makes no
// HIP call, so it runs anywhere, and under the host sanitizers:
//   c++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/spec_rule_host_check.cpp -o spec_rule_host_check
// (tests/test_spec_sample_cpu.py compiles it without the sanitizers and feeds it.)  One query per input line, numbers in hex, one
// answer line each:
//   m z U             mulshift(z, U)                     z up to 128 bits
//   a Px Zp Qx Zq U   spec_accept: 0 or 1
//   r Pi Zp Qi Zq     spec_residual
//   u bits            spec_u24 of the fp32 with these bits
// Exit status 0: every line was understood.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../micromix_amd/csrc/mx_spec_rule.h"

using namespace mm;

static bool parse_hex(const char *s, u128 *out) {
    u128 v = 0;
    if (!*s || strlen(s) > 32) return false;
    for (; *s; ++s) {
        const int d = *s >= '0' && *s <= '9' ? *s - '0' : *s >= 'a' && *s <= 'f' ? *s - 'a' + 10 : -1;
        if (d < 0) return false;
        v = v << 4 | (u128)d;
    }
    *out = v;
    return true;
}

static void print_hex(u128 v) {
    const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
    if (hi) printf("%llx%016llx\n", hi, lo);
    else printf("%llx\n", lo);
}

int main() {
    char line[512], tok[6][64];
    while (fgets(line, sizeof(line), stdin)) {
        const int n = sscanf(line, "%63s %63s %63s %63s %63s %63s", tok[0], tok[1], tok[2], tok[3], tok[4], tok[5]);
        if (n < 1) continue;
        u128 v[5] = {};
        for (int i = 1; i < n; ++i)
            if (!parse_hex(tok[i], &v[i - 1])) return 2;
        const char op = tok[0][0];
        if (op == 'm' && n == 3 && v[1] < (1u << 24)) {
            print_hex(spec_mulshift(v[0], (unsigned)v[1]));
        } else if (op == 'a' && n == 6 && v[4] < (1u << 24)) {
            printf("%d\n", (int)spec_accept((unsigned long long)v[0], (unsigned long long)v[1], (unsigned long long)v[2], (unsigned long long)v[3],
                                            (unsigned)v[4]));
        } else if (op == 'r' && n == 5) {
            print_hex(spec_residual((unsigned long long)v[0], (unsigned long long)v[1], (unsigned long long)v[2], (unsigned long long)v[3]));
        } else if (op == 'u' && n == 2) {
            const uint32_t bits = (uint32_t)v[0];
            float f;
            memcpy(&f, &bits, 4);
            printf("%x\n", spec_u24(f));
        } else {
            return 2;
        }
    }
    return 0;
}
