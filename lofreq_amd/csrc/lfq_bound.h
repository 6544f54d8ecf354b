/*
 * lfq_bound.h -- the binomial tail bound that gates light columns in front of the screen kernel's DP.
 * Host and device: lfq_scan_gate_kernel evaluates it per light column of a batch gated in the scan, lfq_dp_screen_kernel per
 * claimed column of the others (lfq_bound_drops: one decision for both), the host computes p_lo beside the quality tables,
 * and tests/test_bound_gate.py and tests/test_scan_gate.py compile it with the host compiler into a stand-alone program.
 *
 * The count kernel (lfq_count_column_lean) counts, on a fixed subset of a column, n_lo = the observations that are kept
 * rows whatever their allele (base code <= 3, bq >= max(min_bq, min_alt_bq)) and have bq <= LFQ_BOUND_QLO.  It is handed
 * on rounded DOWN to a multiple of 2^LFQ_BOUND_SHIFT (five bits of the internal class byte): m <= n_lo.
 *
 * Why a column with  B = sum_{k=K}^{min(m, K+J)} C(m,k) p_lo^k (1-p_lo)^(m-k),  B * bonf > sig * (1 + slack),  is one the
 * reference prunes (snpcaller.c:950):
 *   - the rows of a column are independent Bernoulli trials; dropping rows and lowering any row's probability can only
 *     lower P(X >= K);
 *   - the m counted rows are kept rows, and under the conditions of the screen's LB form (no merged-quality filter, an
 *     alt base keeps its own quality) each one's merged error probability is  jp >= pm + (1 - pm) pb >= pb >= p_lo,
 *     p_lo = the smallest entry of the bq table over [max(min_bq, min_alt_bq), LFQ_BOUND_QLO];
 *   - so the exact tail >= P(Bin(m, p_lo) >= K) >= B (a partial sum of its non-negative terms -- never 1 - sum: the
 *     threshold is ~3e-9 and the cancellation would be larger than the slack);
 *   - B is at most 2 K + J + 12 multiplications and J additions of positive doubles away from its exact value (1e-16
 *     relative each, the table entries included), which the slack of 1e-6 covers as it does for the screen's own DP.
 * A cell that underflows makes B smaller (0 at worst): the gate then does not fire, it never fires wrongly.
 */
#ifndef LFQ_BOUND_H
#define LFQ_BOUND_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LFQ_BOUND_FN __host__ __device__ static inline
#else
#define LFQ_BOUND_FN static inline
#endif

#define LFQ_BOUND_QLO 31          /* bq <= 31 is a bit test: (bq & 0xE0) == 0 */
#define LFQ_BOUND_SUBSET 2048     /* observations of a column the count kernel looks at (the first trip of its loop) */
#define LFQ_BOUND_SHIFT 6         /* m = (n_lo >> 6) << 6 */
#define LFQ_BOUND_CODES 32        /* five bits */
#define LFQ_BOUND_MAXK 31         /* the widest screen variant */
#define LFQ_BOUND_J 3             /* terms of the tail above the K-th */
#define LFQ_BOUND_NRK (LFQ_BOUND_MAXK + LFQ_BOUND_J + 1)

/* what the gate needs of p_lo: (1 - p_lo)^m for the 32 values m can take, and p_lo / ((1 - p_lo) k) */
struct LfqBoundTab {
    double qm[LFQ_BOUND_CODES];
    double rk[LFQ_BOUND_NRK];     /* [0] unused */
};

/* n_lo -> the five bits that travel, and back: never above n_lo */
LFQ_BOUND_FN uint32_t lfq_bound_code(uint32_t n_lo)
{
    const uint32_t c = n_lo >> LFQ_BOUND_SHIFT;
    return c < LFQ_BOUND_CODES - 1 ? c : LFQ_BOUND_CODES - 1;
}

LFQ_BOUND_FN int lfq_bound_m(uint32_t code) { return (int)(code << LFQ_BOUND_SHIFT); }

/* the smallest table entry over the qualities lo..hi a counted row can have; 0 (gate off) if there is none or it is
 * not a probability the bound can use */
LFQ_BOUND_FN double lfq_bound_p_lo(const double *bq_lut, int lo, int hi)
{
    double p = 2.0;
    for (int q = lo < 0 ? 0 : lo; q <= hi && q < 256; q++) {
        p = bq_lut[q] < p ? bq_lut[q] : p;
    }
    return (p > 0.0 && p < 1.0) ? p : 0.0;
}

/* entry i of either table (a thread of the screen kernel builds one of each); 0 < p_lo < 1 */
LFQ_BOUND_FN double lfq_bound_qm(double p_lo, uint32_t code)
{
    double b = 1.0 - p_lo, r = 1.0;
    for (uint32_t n = (uint32_t)lfq_bound_m(code); n != 0u; n >>= 1) {      /* at most 11 squarings */
        r = (n & 1u) ? r * b : r;
        b = b * b;
    }
    return r;
}

LFQ_BOUND_FN double lfq_bound_rk(double p_lo, int k) { return k > 0 ? p_lo / (1.0 - p_lo) / (double)k : 0.0; }

LFQ_BOUND_FN void lfq_bound_fill(LfqBoundTab *t, double p_lo)
{
    for (uint32_t i = 0; i < LFQ_BOUND_CODES; i++) {
        t->qm[i] = lfq_bound_qm(p_lo, i);
    }
    for (int k = 0; k < LFQ_BOUND_NRK; k++) {
        t->rk[k] = lfq_bound_rk(p_lo, k);
    }
}

/* B for m = lfq_bound_m(code) rows and 1 <= K <= LFQ_BOUND_MAXK: K + J multiplications by (m - k + 1) * rk[k], the running
 * term C(m,k) p^k q^(m-k) <= 1 throughout */
LFQ_BOUND_FN double lfq_bound_tail(const LfqBoundTab *t, uint32_t code, int K)
{
    const int m = lfq_bound_m(code);
    if (K < 1 || K > LFQ_BOUND_MAXK || m < K) {
        return 0.0;
    }
    double term = t->qm[code];
    for (int k = 1; k <= K; k++) {
        term *= (double)(m - k + 1) * t->rk[k];
    }
    double B = term;
    const int kend = m < K + LFQ_BOUND_J ? m : K + LFQ_BOUND_J;
    for (int k = K + 1; k <= kend; k++) {
        term *= (double)(m - k + 1) * t->rk[k];
        B += term;
    }
    return B;
}

/* THE decision: is a light column with the flag byte's statistic `code` and K alt bases dropped before its DP?  Stated once for
 * the two places that make it -- lfq_scan_gate_kernel for a batch gated in the scan, lfq_dp_screen_kernel<.., GATE = true>
 * for the others -- with the same operands in the same order, so that a knife-edge column falls the same way in both:
 * bonf_d is the column's Bonferroni factor (lfq_bonf_of_prefix) as a double, sig_s = sig * (1 + prune_slack), maxk the
 * launched screen variant's MAXK.  A column with K > maxk is not decided here: it goes to the retry kernel ungated. */
LFQ_BOUND_FN bool lfq_bound_drops(const LfqBoundTab *t, uint32_t code, int K, int maxk, double bonf_d, double sig_s)
{
    return code != 0u && K <= maxk && lfq_bound_tail(t, code & (LFQ_BOUND_CODES - 1u), K) * bonf_d > sig_s;
}

#endif
