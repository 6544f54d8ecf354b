/*
 * lfq_bound_check.cpp -- lfq_bound.h on the host, as a stand-alone program (tests/test_bound_gate.py compiles it with the host
 * compiler; not part of the library).  One request per line of standard input, one answer per line of standard output:
 *
 *   T <p_lo> <n_lo> <K>          ->  <code> <m> <B>      the gate's bound for a column with n_lo counted rows
 *   L <lo> <hi> <n> <v0> .. <vn-1>  ->  <p_lo>          lfq_bound_p_lo over a bq table of n entries
 *   D <p_lo> <code> <K> <maxk> <bonf> <sig_s>  ->  0 | 1   lfq_bound_drops: the decision the scan and the screen kernel share
 *                                                           (tests/test_scan_gate.py)
 *
 * Doubles travel as %.17g / %la, so both sides see the same bits.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lfq_bound.h"

int main(void)
{
    char line[1 << 16];
    LfqBoundTab tab;
    double tab_p = -1.0;
    while (fgets(line, sizeof(line), stdin)) {
        char *s = line;
        const char kind = *s++;
        if (kind == 'T') {
            char *e;
            const double p_lo = strtod(s, &e);
            const unsigned long n_lo = strtoul(e, &e, 10);
            const long K = strtol(e, &e, 10);
            if (!(p_lo > 0.0 && p_lo < 1.0)) {
                printf("0 0 0\n");              /* the host switches the gate off */
                continue;
            }
            if (p_lo != tab_p) {
                lfq_bound_fill(&tab, p_lo);
                tab_p = p_lo;
            }
            const uint32_t code = lfq_bound_code((uint32_t)n_lo);
            printf("%u %d %.17g\n", code, lfq_bound_m(code), lfq_bound_tail(&tab, code, (int)K));
        } else if (kind == 'D') {
            char *e;
            const double p_lo = strtod(s, &e);
            const unsigned long code = strtoul(e, &e, 10);
            const long K = strtol(e, &e, 10);
            const long maxk = strtol(e, &e, 10);
            const double bonf_d = strtod(e, &e);
            const double sig_s = strtod(e, &e);
            if (!(p_lo > 0.0 && p_lo < 1.0) || code >= LFQ_BOUND_CODES) {
                return 2;
            }
            if (p_lo != tab_p) {
                lfq_bound_fill(&tab, p_lo);
                tab_p = p_lo;
            }
            printf("%d\n", lfq_bound_drops(&tab, (uint32_t)code, (int)K, (int)maxk, bonf_d, sig_s) ? 1 : 0);
        } else if (kind == 'L') {
            char *e;
            const long lo = strtol(s, &e, 10);
            const long hi = strtol(e, &e, 10);
            const long n = strtol(e, &e, 10);
            if (n < 0 || n > 256) {
                return 2;
            }
            std::vector<double> lut(256, 2.0);  /* entries past the given ones can never be the minimum */
            for (long i = 0; i < n; i++) {
                lut[(size_t)i] = strtod(e, &e);
            }
            printf("%.17g\n", lfq_bound_p_lo(lut.data(), (int)lo, (int)hi));
        } else if (kind != '\n' && kind != '#') {
            return 2;
        }
    }
    return 0;
}
