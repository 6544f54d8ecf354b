/*
 * lfq_viterbi.hip -- `lofreq viterbi` on the device: the reads with an indel of one contig are re-aligned by the reference's
 * full, unbanded three-state Viterbi (viterbi, viterbi.c:99-330) around its fetch_func (lofreq_viterbi.c:107-345).
 *
 * Every floating-point value of the recurrence is a table value (log10 of a transition or an emission probability,
 * computed on the HOST with the host's libm, exactly the reference's expressions) or a sum of two doubles, and every
 * decision is a comparison of such sums.  The kernel does additions, `>` and selects only, in the reference's term order
 * with argmax_d's first-maximum rule (utils.c:87-98); the cells of an anti-diagonal are independent, so the order they are
 * evaluated in does not touch a bit and the result is the reference's, not an approximation of it.
 *
 *   host    classification from the CIGAR (pass-through reads cost no kernel work), q2def (int_median, utils.c:436-457), the
 *           window, the tables; after the kernel left_align_indels (viterbi.c:48-96) and the run-length CIGAR
 *   device  lfq_viterbi_kernel: one wavefront per read, lanes along the query, 64 query rows a strip, one anti-diagonal a
 *           step; termination and trace-back by one lane
 *
 * lfq_readset_viterbi (lfq_readset.hip) realigns the reads of a resident read set through the same stages: the host walks the
 * CIGARs (and the qualities of the reads with an indel) only, lfq_vit_gather_kernel builds query, q2def and windows from the
 * read set's device arrays, and lfq_readset_permute_kernel writes the per-base arrays of the new read set in its read order.
 */
#include "lfq_ctx.h"

#include <map>

#define LFQ_VIT_RWIN 10                     /* lofreq_viterbi.c:46 */
#define LFQ_VIT_IMIN (-2147483648.0)        /* (double)INT_MIN: the reference's border value (viterbi.c:157-169), not -inf */
#define LFQ_VIT_MAXQ 93

/* the nine transition constants of one window length (viterbi.c:127-143), log10 */
struct LfqVitTp {
    double mm, mi, md, im, ii, dm, dd, sm, si;
    double pad_[7];
};

struct LfqVitRead {                         /* one read the kernel works on */
    int64_t base_off;                       /* its query in qletter / qeff */
    int64_t win_off;                        /* its reference window in win */
    int64_t ptr_off;                        /* bytes: its slab of back pointers (chunk-relative) */
    int64_t ho_off;                         /* doubles: its two hand-over rows (chunk-relative) */
    int64_t st_off;                         /* its traced states in states, q + w bytes */
    int32_t q, w;                           /* query and window length */
    int32_t tp_idx;
    int32_t pad_;
};

struct LfqVitOut {
    int32_t k;                              /* what viterbi() returns: the window column the trace-back stopped at */
    int32_t n_states;                       /* states[st_off + q + w - n_states .. st_off + q + w): 1 M, 2 I, 3 D */
    int32_t end_state, pad_;
};

struct LfqVitArgs {
    const LfqVitRead *reads;
    const uint8_t *qletter;                 /* query bases as letters */
    const uint8_t *qeff;                    /* their qualities, q2def in place of a 2 */
    const uint8_t *win;                     /* reference windows, upper case */
    const LfqVitTp *tp;
    const double *emis;                     /* [94][2]: log10(1 - bp), log10(bp / 3.) */
    double ep_ins;                          /* log10(.25) */
    uint8_t *ptr;
    double *ho;
    uint8_t *states;
    LfqVitOut *out;
    int32_t first, n;                       /* reads [first, first + n) */
};

/* bytes of back pointers per 64-row strip: a lane packs four steps into a dword, a step of the wavefront is 64 bytes */
static inline __host__ __device__ int64_t lfq_vit_strip_bytes(int32_t w)
{
    return (int64_t)((w + 63 + 3) / 4) * 256;
}
/* doubles of one hand-over row (M, I, D of every column), padded to whole 128-byte lines */
static inline __host__ __device__ int64_t lfq_vit_ho_row(int32_t w)
{
    return ((int64_t)3 * (w + 1) + 15) / 16 * 16;
}

/* lane l takes lane l - 1's value, lane 0 takes `edge` (DPP wave_shr:1, a lane without a source keeps the old value) */
static __device__ __forceinline__ double lfq_vit_from_left(double own, double edge)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(own), 0x138, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(own), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

static __device__ __forceinline__ double lfq_vit_lane(double v, int lane)
{
    int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

/* One wavefront per read.  Lane l of strip s owns query row i = 64 s + l + 1 and at step t the cell of column k = t - l + 1:
 * V_M[k][i] needs (k - 1, i - 1), V_I[k][i] needs (k, i - 1) -- the left lane's values of two steps and of one step ago, taken
 * with one lane shift per step and kept for the next -- and V_D[k][i] needs (k - 1, i), the lane's own last values.  The row
 * above a strip (row 0: the INT_MIN border) comes from the hand-over row its last lane wrote, 64 columns a load, and enters
 * the shift as lane 0's edge value.  The V_* are never stored; a cell leaves its three back pointers in one byte. */
__global__ __launch_bounds__(256) void lfq_viterbi_kernel(LfqVitArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wv = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wv >= a.n) {
        return;
    }
    const LfqVitRead R = a.reads[a.first + wv];
    const int q = R.q, w = R.w;
    const LfqVitTp tp = a.tp[R.tp_idx];
    const uint8_t *ql = a.qletter + R.base_off, *qe = a.qeff + R.base_off, *win = a.win + R.win_off;
    uint8_t *ptr = a.ptr + R.ptr_off;
    const int64_t ho_row = lfq_vit_ho_row(w), strip_bytes = lfq_vit_strip_bytes(w);
    const int w1 = w + 1;
    const int n_strips = (q + 63) >> 6;
    const double IMIN = LFQ_VIT_IMIN;

    /* termination (viterbi.c:241-255), kept by the lane that owns the last query row while it walks the columns in order */
    double best = IMIN;
    int best_k = 0, end_state = 0;

    for (int s = 0; s < n_strips; s++) {
        const int i = (s << 6) + lane + 1;
        const bool row_on = i <= q;
        const int rows = min(64, q - (s << 6));
        const int n_steps = w + rows - 1;
        const uint8_t qc = row_on ? ql[i - 1] : 0;
        const int qq = row_on ? qe[i - 1] : 0;
        const double ep_m = a.emis[2 * qq], ep_n = a.emis[2 * qq + 1];
        const double v_start = i == 1 ? 0.0 : IMIN;             /* V_start[i - 1] (viterbi.c:157-170) */
        const double s_m = v_start + tp.sm, s_i = v_start + tp.si;
        const double *ho_in = a.ho + R.ho_off + (int64_t)((s + 1) & 1) * ho_row;
        double *ho_out = a.ho + R.ho_off + (int64_t)(s & 1) * ho_row;
        const bool hand_over = s + 1 < n_strips && lane == 63;
        uint8_t *pstrip = ptr + (int64_t)s * strip_bytes;
        double M = IMIN, I = IMIN, D = IMIN;                    /* column 0 of the row (viterbi.c:160-164) */
        double l2M = IMIN, l2I = IMIN, l2D = IMIN;              /* the row above, one column back */
        for (int tb = 0; tb < n_steps; tb += 64) {
            double cM = IMIN, cI = IMIN, cD = IMIN;             /* the row above at column tb + lane + 1 */
            const int kk = tb + lane + 1;
            if (s > 0 && kk <= w) {
                cM = ho_in[kk];
                cI = ho_in[w1 + kk];
                cD = ho_in[2 * w1 + kk];
            }
            for (int tt = 0; tt < 64 && tb + tt < n_steps; tt += 4) {
                uint32_t packed = 0;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int t = tb + tt + u;
                    const int k = t - lane + 1;
                    const double l1M = lfq_vit_from_left(M, lfq_vit_lane(cM, tt + u));
                    const double l1I = lfq_vit_from_left(I, lfq_vit_lane(cI, tt + u));
                    const double l1D = lfq_vit_from_left(D, lfq_vit_lane(cD, tt + u));
                    if (row_on && k >= 1 && k <= w) {
                        /* V_M (viterbi.c:203-213): S, M, I, D of (k - 1, i - 1), first maximum */
                        double bm = s_m;
                        uint32_t pm = 0;
                        const double m1 = l2M + tp.mm, m2 = l2I + tp.im, m3 = l2D + tp.dm;
                        if (m1 > bm) { bm = m1; pm = 1; }
                        if (m2 > bm) { bm = m2; pm = 2; }
                        if (m3 > bm) { bm = m3; pm = 3; }
                        const double nM = (qc == win[k - 1] ? ep_m : ep_n) + bm;
                        /* V_I (:219-224): S, M, I of (k, i - 1) */
                        double bi = s_i;
                        uint32_t pi = 0;
                        const double i1 = l1M + tp.mi, i2 = l1I + tp.ii;
                        if (i1 > bi) { bi = i1; pi = 1; }
                        if (i2 > bi) { bi = i2; pi = 2; }
                        const double nI = a.ep_ins + bi;
                        /* V_D (:228-232): M, D of (k - 1, i) */
                        double bd = M + tp.md;
                        uint32_t pd = 0;
                        const double d1 = D + tp.dd;
                        if (d1 > bd) { bd = d1; pd = 1; }
                        M = nM;
                        I = nI;
                        D = bd;
                        packed |= (pm | (pi << 2) | (pd << 4)) << (8 * u);
                        if (i == q) {                           /* viterbi.c:244-255: M then I, strictly greater */
                            if (M > best) { best = M; best_k = k; end_state = 1; }
                            if (I > best) { best = I; best_k = k; end_state = 2; }
                        }
                        if (hand_over) {
                            ho_out[k] = M;
                            ho_out[w1 + k] = I;
                            ho_out[2 * w1 + k] = D;
                        }
                    }
                    l2M = l1M;
                    l2I = l1I;
                    l2D = l1D;
                }
                ((uint32_t *)pstrip)[(int64_t)((tb + tt) >> 2) * 64 + lane] = packed;
            }
        }
        __threadfence();            /* the hand-over row and the pointers are read by other lanes of this wavefront */
    }

    /* trace-back (viterbi.c:269-301) by the lane of the last row */
    if (lane == ((q - 1) & 63)) {
        const int cap = q + w;
        uint8_t *st = a.states + R.st_off;
        int i = q, k = best_k, cur = end_state, n = 0;
        while (i != 0 && k != 0 && cur != 0) {
            const int l = (i - 1) & 63, t = k + l - 1;
            const uint32_t b = ptr[(int64_t)((i - 1) >> 6) * strip_bytes + ((int64_t)(t >> 2) * 64 + l) * 4 + (t & 3)];
            st[cap - 1 - n] = (uint8_t)cur;
            n++;
            if (cur == 1) {
                cur = b & 3;                        /* "SMID"[index] */
                i--;
                k--;
            } else if (cur == 2) {
                cur = (b >> 2) & 3;                 /* "SMI"[index] */
                i--;
            } else {
                cur = ((b >> 4) & 1) ? 3 : 1;       /* "MD"[index] */
                k--;
            }
        }
        LfqVitOut o;
        o.k = k;
        o.n_states = n;
        o.end_state = end_state;
        o.pad_ = 0;
        a.out[a.first + wv] = o;
    }
}

/* ---- the reads of a resident read set (lfq_readset_viterbi): query, q2def and window built where the bases are ---------- */

struct LfqVitSrc {                          /* one read lfq_vit_gather_kernel works on, beside its LfqVitRead */
    int64_t read;                           /* its index in the read set */
    int32_t lower;                          /* window start */
    int32_t pad_;
};

struct LfqVitGatherArgs {
    const LfqVitRead *reads;
    const LfqVitSrc *src;
    const int64_t *seq_off, *cigar_off;     /* the read set's device arrays */
    const uint32_t *cigar;
    const uint8_t *seq, *qual, *ref;
    uint8_t *qletter, *qeff, *win;          /* what LfqVitArgs takes */
    int32_t n;
    int32_t def_qual;                       /* -q; negative: the median of the read's qualities other than 2 */
};

/* One wavefront per read, lanes along the bases of a CIGAR operation.  The host has checked every read it lists: M = X I D S
 * operations only, their query bases inside the read's span of seq / qual, the window inside the contig, no quality above 93
 * and at least one other than 2.  First walk: the histogram of the qualities other than 2, 94 bins in LDS, and from it
 * int_median (utils.c:436-457) -- element (m - 1) / 2 and element m / 2 of the sorted values are the same one for an odd
 * count, and the mean of two qualities truncates like (a + b) / 2.0 does.  Second walk: letters and qualities. */
__global__ __launch_bounds__(256) void lfq_vit_gather_kernel(LfqVitGatherArgs a)
{
    __shared__ int s_hist[4][96];
    const int lane = threadIdx.x & 63, wl = threadIdx.x >> 6;
    const int wv = blockIdx.x * 4 + wl;
    const bool on = wv < a.n;               /* (no early return: the block's barriers below) */
    int *hist = s_hist[wl];
    for (int v = lane; v < 96; v += 64) {
        hist[v] = 0;
    }
    __syncthreads();
    LfqVitRead R = {};
    LfqVitSrc S = {};
    int64_t s0 = 0, c0 = 0, c1 = 0;
    if (on) {
        R = a.reads[wv];
        S = a.src[wv];
        s0 = a.seq_off[S.read];
        c0 = a.cigar_off[S.read];
        c1 = a.cigar_off[S.read + 1];
    }
    if (on && a.def_qual < 0) {
        int64_t y = s0;
        for (int64_t j = c0; j < c1; j++) {
            const uint32_t cg = a.cigar[j];
            const int op = (int)(cg & 0xf);
            const int64_t len = cg >> 4;
            if (op == 0 || op == 7 || op == 8 || op == 1) {
                for (int64_t b = lane; b < len; b += 64) {
                    const int qv = a.qual[y + b];
                    if (qv != 2 && qv <= LFQ_VIT_MAXQ) {
                        atomicAdd(&hist[qv], 1);
                    }
                }
                y += len;
            } else if (op == 4) {
                y += len;
            }
        }
    }
    __syncthreads();
    int q2def = a.def_qual;
    if (on && a.def_qual < 0) {
        int m = 0;
        for (int v = 0; v <= LFQ_VIT_MAXQ; v++) {
            m += hist[v];
        }
        const int i_lo = (m - 1) / 2, i_hi = m / 2;
        int v_lo = -1, v_hi = -1, seen = 0;
        for (int v = 0; v <= LFQ_VIT_MAXQ; v++) {       /* element i of the sorted values: the first v with more than i up to it */
            seen += hist[v];
            v_lo = (v_lo < 0 && seen > i_lo) ? v : v_lo;
            v_hi = (v_hi < 0 && seen > i_hi) ? v : v_hi;
        }
        q2def = m > 0 ? (v_lo + v_hi) / 2 : 2;
    }
    if (on) {
        int64_t y = s0, z = R.base_off;
        for (int64_t j = c0; j < c1; j++) {
            const uint32_t cg = a.cigar[j];
            const int op = (int)(cg & 0xf);
            const int64_t len = cg >> 4;
            if (op == 0 || op == 7 || op == 8 || op == 1) {
                for (int64_t b = lane; b < len && z + b < R.base_off + R.q; b += 64) {
                    const uint32_t code = a.seq[y + b];
                    const int qv = a.qual[y + b];
                    a.qletter[z + b] = (uint8_t)(code > 15u ? 'N' : LFQ_SEQ_LETTERS[code]);
                    a.qeff[z + b] = (uint8_t)(qv == 2 ? q2def : qv);
                }
                y += len;
                z += len;
            } else if (op == 4) {
                y += len;
            }
        }
        for (int j = lane; j < R.w; j += 64) {
            const uint32_t ch = a.ref[(int64_t)S.lower + j];
            a.win[R.win_off + j] = (uint8_t)(ch >= 'a' && ch <= 'z' ? ch - 32u : ch);       /* strtoupper (:161) */
        }
    }
}

#define LFQ_PERMUTE_ARRAYS 4                /* seq, qual, BI, BD */
struct LfqPermuteArgs {
    const int64_t *new_off;                 /* [n + 1] seq_off of the new order */
    const int64_t *old_start;               /* [n] first base of the read at place j in the source arrays */
    int64_t n_reads, n_bases;
    int32_t n_arrays, pad_;
    const uint8_t *src[LFQ_PERMUTE_ARRAYS];
    uint8_t *dst[LFQ_PERMUTE_ARRAYS];       /* 16-byte aligned, n_bases + 16 bytes */
};

/* Each lane owns 16 aligned output bytes, finds the read of the first one by binary search in the new offsets (as
 * lfq_idq_fill_kernel does) and copies from where that read lies in the source.  Source offsets have no alignment: 16 bytes of
 * one read are one unaligned load that ends inside that read, bytes of a chunk that straddles reads are loaded one by one. */
__global__ __launch_bounds__(256) void lfq_readset_permute_kernel(LfqPermuteArgs A)
{
    const int64_t b0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (b0 >= A.n_bases) {
        return;
    }
    int64_t lo = 0, hi = A.n_reads;             /* new_off[lo] <= b0 < new_off[hi] */
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.new_off[mid] <= b0) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    int64_t r = lo, r_begin = A.new_off[r], r_end = A.new_off[r + 1];
    if (b0 + 16 <= r_end) {
        const int64_t so = A.old_start[r] + (b0 - r_begin);
        for (int k = 0; k < A.n_arrays; k++) {
            uint4 v;
            __builtin_memcpy(&v, A.src[k] + so, 16);
            *(uint4 *)(A.dst[k] + b0) = v;
        }
        return;
    }
    int64_t from[16];                           /* source index of every byte, -1 behind the last base */
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int64_t b = b0 + i;
        from[i] = -1;
        if (b < A.n_bases) {
            while (b >= r_end && r + 1 < A.n_reads) {       /* on to the next read with bases */
                r++;
                r_begin = r_end;
                r_end = A.new_off[r + 1];
            }
            from[i] = A.old_start[r] + (b - r_begin);
        }
    }
    for (int k = 0; k < A.n_arrays; k++) {
        uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t v = from[i] >= 0 ? A.src[k][from[i]] : 0u;
            out[i >> 2] |= v << (8 * (i & 3));
        }
        *(uint4 *)(A.dst[k] + b0) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

/* ---- host ------------------------------------------------------------------------------------------------- */

struct LfqViterbiState {
    /* the result handed out, valid until the next call */
    lfq_viterbi_result res;
    std::vector<int32_t> pos;
    std::vector<uint8_t> status;
    std::vector<int64_t> cigar_off;
    std::vector<uint32_t> cigar;
    /* device memory, grow-only */
    uint8_t *d_in = nullptr, *d_ptr = nullptr, *d_states = nullptr;
    double *d_ho = nullptr;
    int64_t in_bytes = 0, ptr_bytes = 0, ho_doubles = 0, states_bytes = 0;
    int64_t *d_perm = nullptr;              /* lfq_viterbi_permute: where each read of the new order begins in the old one */
    int64_t perm_words = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    lfq_viterbi_times times;
};

static LfqViterbiState *vit_state(lfq_ctx *c)
{
    if (!c->vit) {
        c->vit = new LfqViterbiState();
        memset(&c->vit->times, 0, sizeof(c->vit->times));
    }
    return c->vit;
}

void lfq_viterbi_release(lfq_ctx *c)
{
    LfqViterbiState *s = c->vit;
    if (!s) {
        return;
    }
    if (s->d_in) (void)hipFree(s->d_in);
    if (s->d_ptr) (void)hipFree(s->d_ptr);
    if (s->d_states) (void)hipFree(s->d_states);
    if (s->d_ho) (void)hipFree(s->d_ho);
    if (s->d_perm) (void)hipFree(s->d_perm);
    for (hipEvent_t e : s->ev) {
        if (e) (void)hipEventDestroy(e);
    }
    delete s;
    c->vit = nullptr;
}

/* viterbi.c:114-143 for one window length; L = strlen(ref) + 1 */
static LfqVitTp vit_transitions(int w)
{
    const double alpha = 0.00001, beta = 0.4;
    const double L = (double)(w + 1);
    const double gamma = 1 / (2. * L);
    LfqVitTp t;
    memset(&t, 0, sizeof(t));
    t.mm = log10((1 - 2 * alpha) * (1 - gamma));
    t.mi = log10(alpha * (1 - gamma));
    t.md = log10(alpha * (1 - gamma));
    t.im = log10((1 - beta) * (1 - gamma));
    t.ii = log10(beta * (1 - gamma));
    t.dm = log10(1 - beta);
    t.dd = log10(beta);
    t.sm = log10((1 - alpha) / L);
    t.si = log10(alpha / L);
    return t;
}

/* left_align_indels (viterbi.c:48-96) on the aligned pair; an index in front of the strings (the reference steps back to -1
 * after a shift at 0) changes nothing */
static void vit_left_align(std::vector<char> &ref, std::vector<char> &query)
{
    const int slen = (int)ref.size();
    int i = 0;
    while (i < slen - 1) {
        if (i >= 0 && ref[i] != '*' && query[i] != '*') {
            if (ref[i + 1] == '*') {
                int ilen = 0;
                while (i + 1 + ilen < slen && ref[i + 1 + ilen] == '*') {
                    ilen++;
                }
                if (query[i + ilen] == ref[i]) {
                    ref[i + ilen] = ref[i];
                    ref[i] = '*';
                    i--;
                    continue;
                }
            } else if (query[i + 1] == '*') {
                int dlen = 0;
                while (i + 1 + dlen < slen && query[i + 1 + dlen] == '*') {
                    dlen++;
                }
                if (query[i] == ref[i + dlen]) {
                    query[i + dlen] = query[i];
                    query[i] = '*';
                    i--;
                    continue;
                }
            }
        }
        i++;
    }
}

struct VitHostRead {
    int64_t r;                  /* index in the batch */
    int32_t lower;              /* window start */
    int32_t q, w;
};

/* what the walk over the CIGARs leaves for the kernel and for the host stages behind it */
struct VitPlan {
    std::vector<VitHostRead> work;
    std::vector<LfqVitRead> dev;
    std::vector<LfqVitSrc> src;                 /* resident reads: where lfq_vit_gather_kernel finds each read */
    std::vector<LfqVitTp> tps;
    std::map<int, int> tp_of_w;
    std::vector<uint8_t> qletter, qeff, win;    /* host reads: packed here; resident reads: built on the device */
    int64_t q_total = 0, win_total = 0, st_total = 0;
    bool packed = true;
};

/* f(index into seq / qual) for every query base of read r: the bases of its M = X I operations (lofreq_viterbi.c:178-213) */
template <typename F>
static void vit_for_query(const lfq_baq_reads *rd, int64_t r, F f)
{
    int64_t y = rd->seq_off[r];
    for (int64_t j = rd->cigar_off[r]; j < rd->cigar_off[r + 1]; j++) {
        const int64_t len = rd->cigar[j] >> 4;
        const int op = rd->cigar[j] & 0xf;
        if (op == 0 || op == 7 || op == 8 || op == 1) {
            for (int64_t b = 0; b < len; b++) {
                f(y + b);
            }
            y += len;
        } else if (op == 4) {
            y += len;
        }
    }
}

/* ---- fetch_func's walk over the CIGAR (lofreq_viterbi.c:171-248): status, query, q2def, window.  pack = false (reads that
 * are resident on the device): query, q2def and window are left to lfq_vit_gather_kernel; the host looks at the CIGARs and at
 * the qualities of the reads with an indel only ---- */
static int vit_scan(LfqViterbiState *S, const lfq_baq_reads *rd, int def_qual, bool pack, VitPlan &P)
{
    const int64_t n = rd->n_reads;
    std::vector<int> rem;
    P.packed = pack;
    for (int64_t r = 0; r < n; r++) {
        const int64_t c0 = rd->cigar_off[r], c1 = rd->cigar_off[r + 1], s0 = rd->seq_off[r], s1 = rd->seq_off[r + 1];
        if (c1 < c0 || s1 < s0 || (c1 > c0 && !rd->cigar) || (s1 > s0 && (!rd->seq || !rd->qual))) {
            return LFQ_ERR_INVALID;
        }
        int64_t x = rd->pos[r], y = 0, z = 0;
        int indels = 0;
        bool skipped = false;
        for (int64_t j = c0; j < c1 && !skipped; j++) {
            const int64_t len = rd->cigar[j] >> 4;
            const int op = rd->cigar[j] & 0xf;
            if (op == 0 || op == 7 || op == 8 || op == 1) {             /* M = X, I: query bases (:180-187, 196-203) */
                if (y + len > s1 - s0) {
                    return LFQ_ERR_INVALID;
                }
                y += len;
                z += len;
                if (op == 1) {
                    indels++;
                } else {
                    x += len;
                }
            } else if (op == 2) {                                       /* D (:193-195) */
                x += len;
                indels++;
            } else if (op == 4) {                                       /* S (:204-207) */
                y += len;
            } else {                                                    /* H, and N / P / B: "Not touching read" (:188-192, 208-212) */
                skipped = true;
            }
        }
        uint8_t status = LFQ_VIT_REALIGNED;
        if (skipped) {
            status = LFQ_VIT_SKIPPED_OP;
        } else if (indels == 0) {
            status = LFQ_VIT_NO_INDEL;                                  /* :216 */
        } else {
            rem.clear();                                                /* check_Q2 / remain (:79-105) */
            vit_for_query(rd, r, [&](int64_t b) {
                if (rd->qual[b] != 2) {
                    rem.push_back(rd->qual[b]);
                }
            });
            if (rem.empty()) {
                status = LFQ_VIT_ALL_Q2;                                /* :221 */
            }
        }
        if (status == LFQ_VIT_REALIGNED) {
            int64_t lower = std::max<int64_t>((int64_t)rd->pos[r] - LFQ_VIT_RWIN, 0);           /* :252-255 */
            int64_t upper = std::min<int64_t>(x + LFQ_VIT_RWIN, rd->ref_len);
            if (rd->pos[r] < 0 || upper <= lower || z > 0x3fffffff || upper - lower > 0x3fffffff) {
                return LFQ_ERR_INVALID;
            }
            /* a quality above 93 has no emission: q2def, a given value or a median of these, is then in range as well */
            for (int v : rem) {
                if (v > LFQ_VIT_MAXQ) {
                    return LFQ_ERR_INVALID;
                }
            }
            if (pack) {
                int q2def = def_qual;
                if (q2def < 0) {                                        /* int_median (utils.c:436-457), by counting */
                    int64_t hist[256] = {0};
                    for (int v : rem) {
                        hist[v]++;
                    }
                    const int64_t m = (int64_t)rem.size();
                    auto at = [&](int64_t idx) {                        /* element idx of the sorted qualities */
                        int v = 0;
                        for (int64_t seen = hist[0]; seen <= idx; seen += hist[v]) {
                            v++;
                        }
                        return v;
                    };
                    q2def = m % 2 == 0 ? (int)((at(m / 2) + at(m / 2 - 1)) / 2.0) : at(m / 2);
                }
                vit_for_query(rd, r, [&](int64_t b) {
                    P.qletter.push_back((uint8_t)lfq_seq_letter(rd->seq[b]));
                    P.qeff.push_back(rd->qual[b] == 2 ? (uint8_t)q2def : rd->qual[b]);
                });
                for (int64_t p = lower; p < upper; p++) {
                    P.win.push_back((uint8_t)toupper((unsigned char)rd->ref[p]));               /* strtoupper, :161 */
                }
            } else {
                LfqVitSrc s;
                s.read = r;
                s.lower = (int32_t)lower;
                s.pad_ = 0;
                P.src.push_back(s);
            }
            VitHostRead h;
            h.r = r;
            h.lower = (int32_t)lower;
            h.q = (int32_t)z;
            h.w = (int32_t)(upper - lower);
            LfqVitRead d;
            memset(&d, 0, sizeof(d));
            d.base_off = P.q_total;
            d.win_off = P.win_total;
            d.st_off = P.st_total;
            d.q = h.q;
            d.w = h.w;
            auto it = P.tp_of_w.find(h.w);
            if (it == P.tp_of_w.end()) {
                it = P.tp_of_w.emplace(h.w, (int)P.tps.size()).first;
                P.tps.push_back(vit_transitions(h.w));
            }
            d.tp_idx = it->second;
            P.q_total += h.q;
            P.win_total += h.w;
            P.st_total += (int64_t)h.q + h.w;
            P.work.push_back(h);
            P.dev.push_back(d);
        }
        S->status[r] = status;
        S->pos[r] = rd->pos[r];
    }
    return LFQ_OK;
}

/* ---- the kernels, over the compacted list, in chunks the scratch budget admits: traced states and where each trace ended.
 * res = the device arrays of a resident read set, in the read order of the plan, or null (query and windows come from the
 * plan's host arrays) ---- */
static int vit_launch(lfq_ctx *c, LfqViterbiState *S, VitPlan &P, int def_qual, const LfqReadsDev *res,
                      std::vector<uint8_t> &states, std::vector<LfqVitOut> &outs)
{
    const int64_t nw = (int64_t)P.work.size(), st_total = P.st_total;
    std::vector<LfqVitRead> &dev = P.dev;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    double emis[2 * (LFQ_VIT_MAXQ + 1)];
    for (int qv = 0; qv <= LFQ_VIT_MAXQ; qv++) {                    /* viterbi.c:188-194; SANGERQUAL_TO_PROB, :40 */
        const double bp = pow(10.0, -0.1 * qv);
        emis[2 * qv] = log10(1 - bp);
        emis[2 * qv + 1] = log10(bp / 3.);
    }
    /* one upload: descriptors | tables | sources (resident reads) | query letters | qualities | windows (host reads) */
    const int64_t o_dev = 0, o_tp = lfq_al(o_dev + nw * (int64_t)sizeof(LfqVitRead));
    const int64_t o_em = lfq_al(o_tp + (int64_t)P.tps.size() * (int64_t)sizeof(LfqVitTp));
    const int64_t o_src = lfq_al(o_em + (int64_t)sizeof(emis)), o_ql = lfq_al(o_src + (int64_t)P.src.size() * (int64_t)sizeof(LfqVitSrc));
    const int64_t o_qe = lfq_al(o_ql + P.q_total), o_win = lfq_al(o_qe + P.q_total), o_out = lfq_al(o_win + P.win_total);
    const int64_t in_total = lfq_al(o_out + nw * (int64_t)sizeof(LfqVitOut));
    const int64_t up_total = res ? o_ql : o_out;
    LFQ_TRY(grow(&S->d_in, &S->in_bytes, in_total));
    LFQ_TRY(grow(&S->d_states, &S->states_bytes, st_total));
    /* chunks: as many reads as the budget -- half of the free memory, at most 32 GiB, or LFQ_BAQ_SCRATCH_MB -- holds */
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    int64_t budget = std::min<int64_t>((int64_t)32 << 30, (int64_t)(free_b / 2));
    if (lfq_knobs().baq_scratch_mb >= 0) {
        budget = (int64_t)lfq_knobs().baq_scratch_mb << 20;
    }
    std::vector<int64_t> chunk_begin(1, 0);
    int64_t need_ptr = 0, need_ho = 0, cur_ptr = 0, cur_ho = 0;
    for (int64_t i = 0; i < nw; i++) {
        const int64_t pb = (int64_t)((P.work[i].q + 63) / 64) * lfq_vit_strip_bytes(P.work[i].w);
        const int64_t hb = 2 * lfq_vit_ho_row(P.work[i].w);
        if (i > chunk_begin.back() && cur_ptr + pb + (cur_ho + hb) * 8 > budget) {
            chunk_begin.push_back(i);
            cur_ptr = cur_ho = 0;
        }
        dev[i].ptr_off = cur_ptr;
        dev[i].ho_off = cur_ho;
        cur_ptr += pb;
        cur_ho += hb;
        need_ptr = std::max(need_ptr, cur_ptr);
        need_ho = std::max(need_ho, cur_ho);
    }
    chunk_begin.push_back(nw);
    LFQ_TRY(grow(&S->d_ptr, &S->ptr_bytes, need_ptr));
    LFQ_TRY(grow(&S->d_ho, &S->ho_doubles, need_ho));
    for (hipEvent_t &e : S->ev) {
        if (!e) {
            LFQ_TRY_HIP(hipEventCreate(&e));
        }
    }
    LfqPin<uint8_t> pin(c, (size_t)up_total);
    LFQ_PIN_OK(pin);
    memcpy(pin.data() + o_dev, dev.data(), (size_t)nw * sizeof(LfqVitRead));
    memcpy(pin.data() + o_tp, P.tps.data(), P.tps.size() * sizeof(LfqVitTp));
    memcpy(pin.data() + o_em, emis, sizeof(emis));
    if (res) {
        memcpy(pin.data() + o_src, P.src.data(), P.src.size() * sizeof(LfqVitSrc));
    } else {
        memcpy(pin.data() + o_ql, P.qletter.data(), P.qletter.size());
        memcpy(pin.data() + o_qe, P.qeff.data(), P.qeff.size());
        memcpy(pin.data() + o_win, P.win.data(), P.win.size());
    }
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_in, pin.data(), (size_t)up_total, hipMemcpyHostToDevice, st));
    LfqVitArgs A;
    memset(&A, 0, sizeof(A));
    A.reads = (const LfqVitRead *)(S->d_in + o_dev);
    A.tp = (const LfqVitTp *)(S->d_in + o_tp);
    A.emis = (const double *)(S->d_in + o_em);
    A.qletter = S->d_in + o_ql;
    A.qeff = S->d_in + o_qe;
    A.win = S->d_in + o_win;
    A.ep_ins = log10(.25);                                          /* viterbi.c:130 */
    A.ptr = S->d_ptr;
    A.ho = S->d_ho;
    A.states = S->d_states;
    A.out = (LfqVitOut *)(S->d_in + o_out);
    LFQ_TRY_HIP(hipEventRecord(S->ev[0], st));
    if (res) {
        LfqVitGatherArgs G;
        memset(&G, 0, sizeof(G));
        G.reads = A.reads;
        G.src = (const LfqVitSrc *)(S->d_in + o_src);
        G.seq_off = res->seq_off;
        G.cigar_off = res->cigar_off;
        G.cigar = res->cigar;
        G.seq = res->seq;
        G.qual = res->qual;
        G.ref = res->ref;
        G.qletter = S->d_in + o_ql;
        G.qeff = S->d_in + o_qe;
        G.win = S->d_in + o_win;
        G.n = (int32_t)nw;
        G.def_qual = def_qual;
        hipLaunchKernelGGL(lfq_vit_gather_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, st, G);
        LFQ_TRY_HIP(hipGetLastError());
    }
    for (size_t ch = 0; ch + 1 < chunk_begin.size(); ch++) {
        A.first = (int32_t)chunk_begin[ch];
        A.n = (int32_t)(chunk_begin[ch + 1] - chunk_begin[ch]);
        hipLaunchKernelGGL(lfq_viterbi_kernel, dim3((unsigned)((A.n + 3) / 4)), dim3(256), 0, st, A);
        LFQ_TRY_HIP(hipGetLastError());
        S->times.n_launches++;
    }
    LFQ_TRY_HIP(hipEventRecord(S->ev[1], st));
    states.resize((size_t)st_total);
    LfqPin<uint8_t> pin_out(c, (size_t)(st_total + nw * (int64_t)sizeof(LfqVitOut)));
    LFQ_PIN_OK(pin_out);
    LFQ_TRY_HIP(hipMemcpyAsync(pin_out.data(), S->d_states, (size_t)st_total, hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipMemcpyAsync(pin_out.data() + st_total, S->d_in + o_out, (size_t)nw * sizeof(LfqVitOut),
                               hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    memcpy(states.data(), pin_out.data(), (size_t)st_total);
    memcpy(outs.data(), pin_out.data() + st_total, (size_t)nw * sizeof(LfqVitOut));
    LFQ_TRY_HIP(hipEventElapsedTime(&S->times.ms_kernels, S->ev[0], S->ev[1]));
    return LFQ_OK;
}

/* ---- left_align_indels, the run-length CIGAR with the clips put back, the new position (:262-321); the result arrays ---- */
static int vit_finish(LfqViterbiState *S, const lfq_baq_reads *rd, const VitPlan &P, const std::vector<uint8_t> &states,
                      const std::vector<LfqVitOut> &outs)
{
    const int64_t n = rd->n_reads, nw = (int64_t)P.work.size();
    std::vector<std::vector<uint32_t>> new_cigar((size_t)nw);
    std::vector<int> bad((size_t)LFQ_HOST_PARTS, 0);
    lfq_for_reads(nw, [&](int64_t b, int64_t e, int part) {
        std::vector<char> ar, aq;
        std::vector<uint8_t> ql;
        for (int64_t i = b; i < e; i++) {
            const VitHostRead &h = P.work[(size_t)i];
            const LfqVitRead &d = P.dev[(size_t)i];
            const LfqVitOut &o = outs[(size_t)i];
            const int cap = h.q + h.w;
            int n_mi = 0, n_md = 0;
            if (o.n_states < 0 || o.n_states > cap || o.end_state == 0) {
                bad[part] = 1;
                continue;
            }
            const uint8_t *stv = states.data() + d.st_off + cap - o.n_states;
            for (int j = 0; j < o.n_states; j++) {
                n_mi += stv[j] != 3;
                n_md += stv[j] != 2;
            }
            int qi = h.q - n_mi, k = o.k;                   /* the trace-back ended at (k, qi) */
            if (qi < 0 || k < 0 || k + n_md > h.w) {
                bad[part] = 1;
                continue;
            }
            const uint8_t *query = P.qletter.data() + d.base_off;
            if (!P.packed) {                                /* resident reads: the letters are taken from the read again */
                ql.clear();
                vit_for_query(rd, h.r, [&](int64_t at) { ql.push_back((uint8_t)lfq_seq_letter(rd->seq[at])); });
                query = ql.data();
            }
            ar.resize((size_t)o.n_states);
            aq.resize((size_t)o.n_states);
            for (int j = 0; j < o.n_states; j++) {          /* tmp_ref / tmp_query (viterbi.c:281-296) */
                ar[j] = stv[j] == 2 ? '*' : (char)toupper((unsigned char)rd->ref[(int64_t)h.lower + k++]);
                aq[j] = stv[j] == 3 ? '*' : (char)query[qi++];
            }
            vit_left_align(ar, aq);
            std::vector<uint32_t> &cg = new_cigar[(size_t)i];
            const int64_t c0 = rd->cigar_off[h.r], c1 = rd->cigar_off[h.r + 1];
            if ((rd->cigar[c0] & 0xf) == 4) {               /* soft-clipped in the front (:270-276) */
                cg.push_back(rd->cigar[c0]);
            }
            auto op_of = [&](int j) { return j < o.n_states ? (ar[j] == '*' ? 1u : aq[j] == '*' ? 2u : 0u) : 2u; };
            uint32_t cur = op_of(0), len = 1;               /* an empty alignment reads its terminator: one D (:279-295) */
            for (int j = 1; j < o.n_states; j++) {
                const uint32_t t = op_of(j);
                if (t != cur) {
                    cg.push_back(len << 4 | cur);
                    cur = t;
                    len = 1;
                } else {
                    len++;
                }
            }
            cg.push_back(len << 4 | cur);
            if ((rd->cigar[c1 - 1] & 0xf) == 4) {           /* ... and in the back (:298-304) */
                cg.push_back(rd->cigar[c1 - 1]);
            }
            S->pos[(size_t)h.r] = h.lower + o.k;            /* :316-321 */
        }
    });
    for (int b : bad) {
        if (b) {
            return LFQ_ERR_HIP;                             /* a trace-back that left the matrix: never a valid result */
        }
    }
    int64_t total = 0, wi = 0;
    for (int64_t r = 0; r < n; r++) {
        total += S->status[r] == LFQ_VIT_REALIGNED ? (int64_t)new_cigar[(size_t)wi++].size()
                                                   : rd->cigar_off[r + 1] - rd->cigar_off[r];
    }
    S->cigar.reserve((size_t)total + 1);
    wi = 0;
    for (int64_t r = 0; r < n; r++) {
        const int64_t c0 = rd->cigar_off[r], c1 = rd->cigar_off[r + 1];
        if (S->status[r] == LFQ_VIT_REALIGNED) {
            const std::vector<uint32_t> &cg = new_cigar[(size_t)wi++];
            const bool same = S->pos[r] == rd->pos[r] && (int64_t)cg.size() == c1 - c0
                              && std::equal(cg.begin(), cg.end(), rd->cigar + c0);
            if (!same) {
                S->status[r] |= LFQ_VIT_CHANGED;
            }
            S->cigar.insert(S->cigar.end(), cg.begin(), cg.end());
        } else if (c1 > c0) {
            S->cigar.insert(S->cigar.end(), rd->cigar + c0, rd->cigar + c1);
        }
        S->cigar_off[r + 1] = (int64_t)S->cigar.size();
    }
    S->cigar.push_back(0);                                  /* never an empty array behind the pointer */
    S->res.n_reads = n;
    S->res.pos = S->pos.data();
    S->res.status = S->status.data();
    S->res.cigar_off = S->cigar_off.data();
    S->res.cigar = S->cigar.data();
    return LFQ_OK;
}

/* lfq_viterbi_batch (res = null), and the realignment of lfq_readset_viterbi: rd = the host arrays the read set was made
 * from, res = its device copies */
int lfq_viterbi_run(lfq_ctx *c, const lfq_baq_reads *rd, int def_qual, const LfqReadsDev *res, const lfq_viterbi_result **out)
{
    if (!c || !rd || !out || rd->n_reads < 0 || def_qual > LFQ_VIT_MAXQ) {
        return LFQ_ERR_INVALID;
    }
    const int64_t n = rd->n_reads;
    if (n > 0 && (!rd->pos || !rd->cigar_off || !rd->seq_off || !rd->ref || rd->ref_len <= 0)) {
        return LFQ_ERR_INVALID;
    }
    LfqViterbiState *S = vit_state(c);
    *out = nullptr;
    S->pos.assign(n, 0);
    S->status.assign(n, LFQ_VIT_NO_INDEL);
    S->cigar_off.assign(n + 1, 0);
    S->cigar.clear();
    memset(&S->times, 0, sizeof(S->times));
    S->times.n_reads = n;
    VitPlan P;
    LFQ_TRY(vit_scan(S, rd, def_qual, res == nullptr, P));
    const int64_t nw = (int64_t)P.work.size();
    std::vector<uint8_t> states;
    std::vector<LfqVitOut> outs((size_t)nw);
    S->times.n_realigned = nw;
    if (nw > 0) {
        LFQ_TRY(vit_launch(c, S, P, def_qual, res, states, outs));
    }
    LFQ_TRY(vit_finish(S, rd, P, states, outs));
    *out = &S->res;
    return LFQ_OK;
}

extern "C" int lfq_viterbi_batch(lfq_ctx *c, const lfq_baq_reads *rd, int def_qual, const lfq_viterbi_result **out)
{
    return lfq_viterbi_run(c, rd, def_qual, nullptr, out);
}

/* the per-base arrays of a read set in a new read order (lfq_readset_viterbi): old_start[j] = where the read at place j begins in
 * the source arrays (host; it goes down here), new_off = the seq_off of the new order on the device */
int lfq_viterbi_permute(lfq_ctx *c, int64_t n_reads, int64_t n_bases, const int64_t *d_new_off, const int64_t *old_start,
                        int n_arrays, const uint8_t *const *src, uint8_t *const *dst)
{
    if (n_reads <= 0 || n_bases <= 0 || n_arrays <= 0) {
        return LFQ_OK;
    }
    if (n_arrays > LFQ_PERMUTE_ARRAYS) {
        return LFQ_ERR_INVALID;
    }
    LfqViterbiState *S = vit_state(c);
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(grow(&S->d_perm, &S->perm_words, n_reads));
    LfqPin<int64_t> pin(c, (size_t)n_reads);
    LFQ_PIN_OK(pin);
    memcpy(pin.data(), old_start, (size_t)n_reads * sizeof(int64_t));
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_perm, pin.data(), (size_t)n_reads * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    LfqPermuteArgs A;
    memset(&A, 0, sizeof(A));
    A.new_off = d_new_off;
    A.old_start = S->d_perm;
    A.n_reads = n_reads;
    A.n_bases = n_bases;
    A.n_arrays = n_arrays;
    for (int a = 0; a < n_arrays; a++) {
        A.src[a] = src[a];
        A.dst[a] = dst[a];
    }
    const int64_t blocks = ((n_bases + 15) / 16 + 255) / 256;
    hipLaunchKernelGGL(lfq_readset_permute_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY_HIP(hipStreamSynchronize(c->stream));          /* (the pinned offsets go back to the pool) */
    return LFQ_OK;
}

extern "C" int lfq_last_viterbi_times(lfq_ctx *c, lfq_viterbi_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = vit_state(c)->times;
    return LFQ_OK;
}
