/*
 * lfq_vcf.hip -- VCF text parsed on the device and `lofreq vcfset` (include/lofreq_amd.h: lfq_vcf_*, lfq_vcfset), over lfq_vcf.h.
 *
 *   scan     three launches over the resident bytes, a lane per chunk of 16 aligned bytes (one dwordx4 load, lfq_fasta.h's masks):
 *              tiles   the line-starting newlines of a chunk, summed per workgroup
 *              sums    one wavefront scans the tiles' sums, LFQ_VCF_SCAN_LANES tiles a round
 *              emit    the masks again: every line's start goes to its slot; a NUL reports its line, a line that starts with the
 *                      #CHROM prefix its number (atomic minima: the same answer whatever order the lanes ran in)
 *   parse    a lane per line: lfq_vc_parse_line on aligned dwords, up to INFO's tab.  The end of the records (stream mode) is an
 *            atomic minimum over the lines with fewer than five fields.
 *   runs     a lane per record: is its CHROM the previous record's?  Run heads -> a scan -> run ids.  Tabix mode: POS order inside a
 *            run, POS >= 1, REF, END=.  The host reads the heads' names only.
 *   exscan / scatter   the scan every list here is made by: one workgroup walks the values 8 192 a round.  No atomic decides a place.
 *   info     a lane per record: DP, SB, DP4 and where AF's value stands (the host runs strtof on those bytes).
 *   match    a lane per record of file 1: lfq_vc_var1, then a binary search in file 2's run and a walk over the equal positions.
 *   plan     a lane per record: the written line's length.  Offsets by exscan.
 *   copy     output-major: a lane owns 16 aligned output bytes and one 16-byte store; it finds its record by binary search in the
 *            offsets and takes every byte from lfq_vc_piece_byte.
 *   mask     a lane per record of a run: byte pos of the -S mask, under a BED only where lfq_bed.h's predicate holds.
 */
#include "lfq_ctx.h"
#include "lfq_vcf.h"

#define LFQ_VCF_CHUNK 16
#define LFQ_VCF_THREADS 256
#define LFQ_VCF_TILE 4096
#define LFQ_VCF_SCAN_LANES 64
#define LFQ_VCF_SCAN_THREADS 1024
#define LFQ_VCF_SCAN_ITEMS 8
static_assert(LFQ_VCF_CHUNK == LFQ_FA_CHUNK && LFQ_VCF_TILE == LFQ_VCF_THREADS * LFQ_VCF_CHUNK, "the chunk masks are lfq_fasta.h's");

#define VC_NONE 0xffffffffffffffffull

/* what the kernels of lfq_vcf_open fill in: the table of lfq_vcf.h with pointers that may be written */
struct LfqVcDev {
    LfqVcTab T;
    int64_t n_chunks, n_tiles;
    int64_t *tile_nl;                   /* [n_tiles + 1] */
    int64_t *lstart, *pos;
    uint16_t *off;
    uint8_t *nf, *flags;
    int32_t *qual;
    int32_t *val;                       /* [n_lines] what the next exscan sums */
    int64_t *ex;                        /* [n_lines + 1] */
    unsigned long long *atom;           /* [0] the header line, [1] the end of the records, [2] line * 8 + why */
};

__device__ __forceinline__ uint32_t vc_wave_incl(uint32_t x)
{
    const int lane = (int)(threadIdx.x & 63);
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) {
            x += y;
        }
    }
    return x;
}

/* exclusive scan of v over a workgroup of LFQ_VCF_THREADS; *total: the workgroup's sum.  Once per kernel */
__device__ __forceinline__ uint32_t vc_block_exscan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const int wv = (int)(threadIdx.x >> 6);
    const uint32_t x = vc_wave_incl(v);
    if ((threadIdx.x & 63) == 63) {
        s_w[wv] = x;
    }
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int i = 0; i < LFQ_VCF_THREADS / 64; i++) {
        base += i < wv ? s_w[i] : 0;
        all += s_w[i];
    }
    *total = all;
    return base + x - v;
}

struct LfqVcChunk {
    uint32_t starts, nul;               /* masks: newlines that start a line; NUL bytes of the file */
};

__device__ __forceinline__ LfqVcChunk vc_chunk(const LfqVcDev &D, int64_t c)
{
    const uint4 w = *reinterpret_cast<const uint4 *>(D.T.text + c * LFQ_VCF_CHUNK);
    const LfqFaMasks m = lfq_fa_chunk_masks(w.x, w.y, w.z, w.w);
    LfqVcChunk k;
    k.starts = lfq_fa_line_starts(m.nl, c, D.T.n);
    k.nul = lfq_fa_nibble(lfq_fa_eq_hi(w.x, 0)) | (lfq_fa_nibble(lfq_fa_eq_hi(w.y, 0)) << 4) | (lfq_fa_nibble(lfq_fa_eq_hi(w.z, 0)) << 8)
            | (lfq_fa_nibble(lfq_fa_eq_hi(w.w, 0)) << 12);
    const int64_t left = D.T.n - c * LFQ_VCF_CHUNK;                     /* the padding behind the file is no NUL of the file */
    if (left < LFQ_VCF_CHUNK) {
        k.nul &= (1u << left) - 1u;
    }
    return k;
}

__global__ __launch_bounds__(LFQ_VCF_THREADS) void lfq_vcf_tiles_kernel(LfqVcDev D)
{
    __shared__ uint32_t s_w[LFQ_VCF_THREADS / 64];
    const int64_t c = (int64_t)blockIdx.x * LFQ_VCF_THREADS + threadIdx.x;
    uint32_t total;
    (void)vc_block_exscan(c < D.n_chunks ? (uint32_t)__popc(vc_chunk(D, c).starts) : 0u, s_w, &total);
    if (threadIdx.x == 0) {
        D.tile_nl[blockIdx.x] = total;
    }
}

/* one wavefront: the sums per tile -> exclusive bases, in place; slot n_tiles gets the total */
__global__ __launch_bounds__(LFQ_VCF_SCAN_LANES) void lfq_vcf_sums_kernel(LfqVcDev D)
{
    int64_t base = 0;
    for (int64_t t0 = 0; t0 < D.n_tiles; t0 += LFQ_VCF_SCAN_LANES) {
        const int64_t t = t0 + threadIdx.x;
        const uint32_t in = t < D.n_tiles ? (uint32_t)D.tile_nl[t] : 0u;   /* (a tile has at most 4 096 newlines) */
        const uint32_t inc = vc_wave_incl(in);
        if (t < D.n_tiles) {
            D.tile_nl[t] = base + inc - in;
        }
        base += __shfl(inc, 63, 64);
    }
    if (threadIdx.x == 0) {
        D.tile_nl[D.n_tiles] = base;
    }
}

__global__ __launch_bounds__(LFQ_VCF_THREADS) void lfq_vcf_emit_kernel(LfqVcDev D, int mode)
{
    __shared__ uint32_t s_w[LFQ_VCF_THREADS / 64];
    const int64_t c = (int64_t)blockIdx.x * LFQ_VCF_THREADS + threadIdx.x;
    LfqVcChunk k = {0, 0};
    if (c < D.n_chunks) {
        k = vc_chunk(D, c);
    }
    uint32_t total;
    const uint32_t ex = vc_block_exscan((uint32_t)__popc(k.starts), s_w, &total);
    const int64_t nl0 = D.tile_nl[blockIdx.x] + ex;                     /* line-starting newlines in front of the chunk */
    int64_t nl = nl0;
    for (uint32_t m = k.starts; m; m &= m - 1) {
        const int i = __ffs((int)m) - 1;
        const int64_t s = c * LFQ_VCF_CHUNK + i + 1;                    /* s < n: the file's last byte starts no line */
        D.lstart[1 + nl] = s;                                           /* (1 + nl <= n_lines - 1: by the count of the same mask) */
        if (mode == LFQ_VC_STREAM && 1 + nl < LFQ_VCF_MAX_HEADER_LINES && lfq_vc_is_header_line(D.T.text, s, D.T.n)) {
            atomicMin(&D.atom[0], (unsigned long long)(1 + nl));
        }
        nl++;
    }
    if (k.nul) {
        const int i = __ffs((int)k.nul) - 1;                            /* the chunk's first NUL is in its earliest such line */
        atomicMin(&D.atom[2], (unsigned long long)(nl0 + __popc(k.starts & ((1u << i) - 1u))) * 8ull + LFQ_VC_NUL);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        D.lstart[0] = 0;
        D.lstart[D.T.n_lines] = D.T.text[D.T.n - 1] == '\n' ? D.T.n : D.T.n + 1;
        if (mode == LFQ_VC_STREAM && lfq_vc_is_header_line(D.T.text, 0, D.T.n)) {
            atomicMin(&D.atom[0], 0ull);
        }
    }
}

__global__ __launch_bounds__(256) void lfq_vcf_parse_kernel(LfqVcDev D, int mode)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= D.T.n_lines) {
        return;
    }
    const int64_t s = D.lstart[k], e = D.lstart[k + 1] - 1;
    LfqVcLine L;
    if (e - s > LFQ_VCF_MAX_LINE) {                                     /* decided from the offsets: the line is not walked */
        atomicMin(&D.atom[2], (unsigned long long)k * 8ull + LFQ_VC_LINE_TOO_LONG);
        for (int j = 0; j < LFQ_VC_NOFF; j++) {
            L.off[j] = 0;
        }
        L.nf = 0;
        L.flags = D.T.text[s] == '#' ? LFQ_VC_F_HASH : 0;
        L.qual = -1;
        L.pos = -1;
    } else {
        lfq_vc_parse_line(D.T.text, s, e, &L);
    }
#pragma unroll
    for (int j = 0; j < LFQ_VC_NOFF; j++) {
        D.off[k * LFQ_VC_NOFF + j] = L.off[j];
    }
    D.nf[k] = L.nf;
    D.flags[k] = L.flags;
    D.qual[k] = L.qual;
    D.pos[k] = L.pos;
    if (mode == LFQ_VC_STREAM) {
        const unsigned long long h = D.atom[0];                         /* (written by the launch before this one) */
        if (L.nf < 5 && k >= (h == VC_NONE ? 0 : (int64_t)h + 1)) {
            atomicMin(&D.atom[1], (unsigned long long)k);
        }
    } else {
        const bool rec = !(L.flags & LFQ_VC_F_HASH) && L.nf >= 5;
        D.val[k] = rec ? 1 : 0;
        if (!(L.flags & LFQ_VC_F_HASH) && L.nf < 5 && e - s <= LFQ_VCF_MAX_LINE) {
            atomicMin(&D.atom[2], (unsigned long long)k * 8ull + LFQ_VC_FIELDS);
        }
    }
}

/* ex[i] = val[0] + .. + val[i - 1], ex[n] the sum: ONE workgroup, LFQ_VCF_SCAN_THREADS * LFQ_VCF_SCAN_ITEMS values a round */
__global__ __launch_bounds__(LFQ_VCF_SCAN_THREADS) void lfq_vcf_exscan_kernel(const int32_t *__restrict__ val, int64_t n, int64_t *__restrict__ ex)
{
    __shared__ int64_t s_w[LFQ_VCF_SCAN_THREADS / 64];
    __shared__ int64_t s_base;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) {
        s_base = 0;
    }
    __syncthreads();
    for (int64_t i0 = 0; i0 < n; i0 += LFQ_VCF_SCAN_THREADS * LFQ_VCF_SCAN_ITEMS) {
        const int64_t i = i0 + (int64_t)threadIdx.x * LFQ_VCF_SCAN_ITEMS;      /* a thread owns LFQ_VCF_SCAN_ITEMS neighbours */
        int32_t mine[LFQ_VCF_SCAN_ITEMS];
        int64_t v = 0;
#pragma unroll
        for (int j = 0; j < LFQ_VCF_SCAN_ITEMS; j++) {
            mine[j] = i + j < n ? val[i + j] : 0;
            v += mine[j];
        }
        int64_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)x, d, 64), hi = __shfl_up((uint32_t)((uint64_t)x >> 32), d, 64);
            if (lane >= d) {
                x += (int64_t)(((uint64_t)hi << 32) | lo);
            }
        }
        if (lane == 63) {
            s_w[wv] = x;
        }
        __syncthreads();
        int64_t base = s_base, all = 0;
        for (int w = 0; w < LFQ_VCF_SCAN_THREADS / 64; w++) {
            base += w < wv ? s_w[w] : 0;
            all += s_w[w];
        }
        int64_t at = base + x - v;
#pragma unroll
        for (int j = 0; j < LFQ_VCF_SCAN_ITEMS; j++) {
            if (i + j < n) {
                ex[i + j] = at;
            }
            at += mine[j];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            s_base += all;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ex[n] = s_base;
    }
}

/* the elements with val != 0, in order: list[ex[i]] = i; rank_or_null[i] = how many such stand at or in front of i, minus one */
__global__ __launch_bounds__(256) void lfq_vcf_scatter_kernel(const int32_t *__restrict__ val, const int64_t *__restrict__ ex, int64_t n,
                                                              int64_t *__restrict__ list, int32_t *__restrict__ rank_or_null)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    if (val[i]) {
        list[ex[i]] = i;                                                /* ex[i] < ex[n]: the list's length */
    }
    if (rank_or_null) {
        rank_or_null[i] = (int32_t)(ex[i] + (val[i] ? 1 : 0) - 1);
    }
}

__global__ __launch_bounds__(256) void lfq_vcf_runs_kernel(LfqVcDev D, int mode)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= D.T.n_rec) {
        return;
    }
    const int64_t k = lfq_vc_line_of(D.T, r), kp = r > 0 ? lfq_vc_line_of(D.T, r - 1) : -1;
    if (D.T.flags[k] & LFQ_VC_F_NUMBER) {
        atomicMin(&D.atom[2], (unsigned long long)k * 8ull + LFQ_VC_NUMBER);
    }
    const bool head = r == 0 || !lfq_vc_field_equal(D.T, k, D.T, kp, 0);
    D.val[r] = head ? 1 : 0;
    if (mode == LFQ_VC_TABIX) {
        if (!lfq_vc_interval_ok(D.T, k)) {
            atomicMin(&D.atom[2], (unsigned long long)k * 8ull + LFQ_VC_INTERVAL);
        }
        if (!head && D.T.pos[k] < D.T.pos[kp]) {
            atomicMin(&D.atom[2], (unsigned long long)k * 8ull + LFQ_VC_UNSORTED);
        }
    }
}

struct LfqVcHead {
    int64_t line, name_beg;
    int32_t name_len, pad_;
};

__global__ __launch_bounds__(256) void lfq_vcf_heads_kernel(LfqVcDev D, LfqVcHead *__restrict__ out)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= D.T.n_runs) {
        return;
    }
    const int64_t k = lfq_vc_line_of(D.T, D.T.run_beg[h]);
    out[h].line = k;
    out[h].name_beg = D.T.lstart[k];
    out[h].name_len = lfq_vc_fend(D.T.off + k * LFQ_VC_NOFF, 0);
    out[h].pad_ = 0;
}

__global__ __launch_bounds__(256) void lfq_vcf_info_kernel(LfqVcTab T, LfqVcInfo *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= T.n_rec) {
        return;
    }
    LfqVcInfo I;
    lfq_vc_info_values(T, lfq_vc_line_of(T, r), &I);
    out[r] = I;
}

/* counters: [0] n_vars1, [1] n_ignored, [2] n_out (sums: their order does not matter); bad: (file << 40 | line) * 8 + why */
__global__ __launch_bounds__(256) void lfq_vcf_match_kernel(LfqVcTab A, LfqVcTab B, const int64_t *__restrict__ run_map, LfqVcSetConf conf,
                                                            int file, uint8_t *__restrict__ keep, unsigned long long *__restrict__ counters,
                                                            unsigned long long *__restrict__ bad)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int code = LFQ_VC_K_DROPPED;
    if (r < A.n_rec) {
        const int64_t k = lfq_vc_line_of(A, r);
        code = lfq_vc_var1(A.flags[k], conf);
        if (code < 0) {
            atomicMin(bad, (((unsigned long long)file << 40) | (unsigned long long)k) * 8ull + LFQ_VC_MULTIALLELIC);
            code = LFQ_VC_K_DROPPED;
        } else if (code == LFQ_VC_K_TAKEN && conf.op != LFQ_VC_OP_CONCAT && A.pos[k] < 0) {
            atomicMin(bad, (((unsigned long long)file << 40) | (unsigned long long)k) * 8ull + LFQ_VC_INTERVAL);
        } else if (code == LFQ_VC_K_TAKEN) {
            const bool m = conf.op == LFQ_VC_OP_CONCAT
                           || lfq_vc_match(A, k, B, run_map[A.run_id[r]], conf) == (conf.op == LFQ_VC_OP_INTERSECT);
            code = m ? LFQ_VC_K_WRITTEN : LFQ_VC_K_TAKEN;
        }
        keep[r] = (uint8_t)code;
    }
    const unsigned long long b1 = __ballot(code >= LFQ_VC_K_TAKEN), b2 = __ballot(code == LFQ_VC_K_IGNORED),
                             b3 = __ballot(code == LFQ_VC_K_WRITTEN);
    if ((threadIdx.x & 63) == 0) {
        if (b1) atomicAdd(&counters[0], (unsigned long long)__popcll(b1));
        if (b2) atomicAdd(&counters[1], (unsigned long long)__popcll(b2));
        if (b3) atomicAdd(&counters[2], (unsigned long long)__popcll(b3));
    }
}

__global__ __launch_bounds__(256) void lfq_vcf_plan_kernel(LfqVcTab A, const uint8_t *__restrict__ keep, int add_len, int32_t *__restrict__ val)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rec) {
        return;
    }
    int32_t len = 0;
    if (keep[r] == LFQ_VC_K_WRITTEN) {
        LfqVcPieces P;
        lfq_vc_pieces(A, lfq_vc_line_of(A, r), add_len, &P);
        len = P.total;
    }
    val[r] = len;
}

/* the lines of one file stand at out[base, base + ex[n_rec]); chunk g of `out` is [16 g, 16 g + 16) */
__global__ __launch_bounds__(256) void lfq_vcf_copy_kernel(LfqVcTab A, const int64_t *__restrict__ ex, int64_t base, const char *__restrict__ add,
                                                           int add_len, uint8_t *__restrict__ out)
{
    const int64_t total = ex[A.n_rec];
    const int64_t g = base / 16 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t lo = max(g * 16, base), hi = min(g * 16 + 16, base + total);
    if (lo >= hi) {
        return;
    }
    int64_t a = 0, b = A.n_rec;         /* -> the last record with ex[r] <= lo - base: the one that holds the byte */
    while (b - a > 1) {
        const int64_t mid = a + ((b - a) >> 1);
        if (ex[mid] <= lo - base) {
            a = mid;
        } else {
            b = mid;
        }
    }
    int64_t r = a;
    LfqVcPieces P;
    lfq_vc_pieces(A, lfq_vc_line_of(A, r), add_len, &P);
    int32_t q = (int32_t)(lo - base - ex[r]);
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int64_t p = g * 16 + j;
        if (p >= lo && p < hi) {
            if (q >= P.total) {         /* the next record that is written (one exists: p < base + total) */
                do {
                    r++;
                } while (ex[r + 1] == ex[r]);
                lfq_vc_pieces(A, lfq_vc_line_of(A, r), add_len, &P);
                q = 0;
            }
            o[j >> 2] |= ((uint32_t)lfq_vc_piece_byte(A, P, q, add) & 0xffu) << ((j & 3) * 8);
            q++;
        }
    }
    if (hi - lo == 16) {
        *reinterpret_cast<uint4 *>(out + g * 16) = make_uint4(o[0], o[1], o[2], o[3]);
        return;
    }
    for (int64_t p = lo; p < hi; p++) {                                 /* the file's first and last chunk: no byte outside its lines */
        const int j = (int)(p - g * 16);
        out[p] = (uint8_t)(o[j >> 2] >> ((j & 3) * 8));
    }
}

/* records [r0, r1): one run.  bed.n < 0: no BED */
__global__ __launch_bounds__(256) void lfq_vcf_mask_kernel(LfqVcTab T, int64_t r0, int64_t r1, int64_t ref_len, LfqBedTab bed,
                                                           uint8_t *__restrict__ mask)
{
    const int64_t r = r0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= r1) {
        return;
    }
    const int64_t p = T.pos[lfq_vc_line_of(T, r)];
    if (!lfq_vc_mask_hit(p, ref_len, bed)) {
        return;
    }
    mask[p] = 1;                        /* (equal values: the stores of two lanes race harmlessly) */
}

/* ---- host ---------------------------------------------------------------------------------------------------------------------------- */
struct lfq_vcf {
    lfq_ctx *c;
    int mode;
    LfqVcDev D;
    uint8_t *d_text, *d_tab, *d_rec;
    int64_t hdr_line, lines_behind;
    std::string header;
    std::vector<std::string> run_name;
    std::vector<int64_t> run_beg;
    /* host copies, made on first request */
    bool have_table, have_text;
    std::vector<uint8_t> h_text, h_flags, h_nf;
    std::vector<int64_t> h_lstart, h_pos, h_line;
    std::vector<int32_t> h_qual, h_run_id;
    std::vector<uint16_t> h_off;
    std::vector<const char *> h_names;
    /* what lfq_vcf_uniq_variants handed out last */
    std::vector<int64_t> u_pos, u_ref_off, u_alt_off, u_line;
    std::string u_ref, u_alt;
    std::vector<uint8_t> u_key;
    std::vector<float> u_af;
};

struct LfqVcfState {
    lfq_vcf_times times;
    LfqEvPair scan_t, parse_t, info_t, match_t, emit_t;
    bool scan_on, parse_on, info_on, match_on, emit_on;
    lfq_vcfset_result res;
    std::vector<uint8_t> keep;
    uint8_t *h_text;
    int64_t h_text_cap;
    uint8_t *d_work, *d_out;            /* lfq_vcfset's scratch and output on the device: the context's own, grow only */
    int64_t d_work_cap, d_out_cap;
};

static LfqVcfState *vc_state(lfq_ctx *c)
{
    if (!c->vcf) {
        LfqVcfState *S = new LfqVcfState();
        memset(&S->times, 0, sizeof(S->times));
        for (LfqEvPair *t : {&S->scan_t, &S->parse_t, &S->info_t, &S->match_t, &S->emit_t}) {
            memset(t->ev, 0, sizeof(t->ev));
        }
        S->scan_on = S->parse_on = S->info_on = S->match_on = S->emit_on = false;
        memset(&S->res, 0, sizeof(S->res));
        S->h_text = S->d_work = S->d_out = nullptr;
        S->d_work_cap = S->d_out_cap = 0;
        S->h_text_cap = 0;
        c->vcf = S;
    }
    return c->vcf;
}

void lfq_vcf_release(lfq_ctx *c)
{
    if (LfqVcfState *S = c->vcf) {
        for (LfqEvPair *t : {&S->scan_t, &S->parse_t, &S->info_t, &S->match_t, &S->emit_t}) {
            t->destroy();
        }
        free_pinned(&S->h_text, &S->h_text_cap);
        if (S->d_work) (void)hipFree(S->d_work);
        if (S->d_out) (void)hipFree(S->d_out);
        delete S;
        c->vcf = nullptr;
    }
}

void lfq_vcf_view(const lfq_vcf *v, lfq_ctx **c, int *mode, LfqVcTab *T, const std::vector<std::string> **names)
{
    *c = v->c;
    *mode = v->mode;
    *T = v->D.T;
    *names = &v->run_name;
}

static inline unsigned vc_grid(int64_t n) { return (unsigned)((std::max<int64_t>(n, 1) + 255) / 256); }
static bool vc_launched() { return hipGetLastError() == hipSuccess; }

/* val[0, n) -> ex[0, n]; the sum comes back */
static int vc_exscan(lfq_vcf *v, int64_t n, int64_t *sum, LfqVcfState *S)
{
    hipStream_t st = v->c->stream;
    hipLaunchKernelGGL(lfq_vcf_exscan_kernel, dim3(1), dim3(LFQ_VCF_SCAN_THREADS), 0, st, v->D.val, n, v->D.ex);
    S->times.n_launches += 1;
    if (!vc_launched() || hipMemcpyAsync(sum, v->D.ex + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess
        || hipStreamSynchronize(st) != hipSuccess) {
        return LFQ_ERR_HIP;
    }
    return LFQ_OK;
}

static int vc_host_text(lfq_vcf *v)
{
    if (!v->have_text && v->D.T.n > 0) {
        v->h_text.resize((size_t)v->D.T.n);
        LFQ_TRY_HIP(hipSetDevice(v->c->device));
        LFQ_TRY_HIP(hipMemcpy(v->h_text.data(), v->d_text, (size_t)v->D.T.n, hipMemcpyDeviceToHost));
    }
    v->have_text = true;
    return LFQ_OK;
}

static int vc_host_table(lfq_vcf *v)
{
    if (v->have_table) {
        return LFQ_OK;
    }
    const LfqVcTab &T = v->D.T;
    const int64_t nl = T.n_lines, nr = T.n_rec;
    v->h_line.resize((size_t)nr);
    v->h_run_id.resize((size_t)nr);
    if (nl > 0) {
        LFQ_TRY_HIP(hipSetDevice(v->c->device));
        std::vector<int64_t> pos((size_t)nl);
        std::vector<int32_t> qual((size_t)nl);
        std::vector<uint8_t> nf((size_t)nl), flags((size_t)nl);
        std::vector<uint16_t> off((size_t)nl * LFQ_VC_NOFF);
        v->h_lstart.resize((size_t)nl + 1);
        LFQ_TRY_HIP(hipMemcpy(v->h_lstart.data(), T.lstart, (size_t)(nl + 1) * 8, hipMemcpyDeviceToHost));
        LFQ_TRY_HIP(hipMemcpy(pos.data(), T.pos, (size_t)nl * 8, hipMemcpyDeviceToHost));
        LFQ_TRY_HIP(hipMemcpy(qual.data(), T.qual, (size_t)nl * 4, hipMemcpyDeviceToHost));
        LFQ_TRY_HIP(hipMemcpy(nf.data(), T.nf, (size_t)nl, hipMemcpyDeviceToHost));
        LFQ_TRY_HIP(hipMemcpy(flags.data(), T.flags, (size_t)nl, hipMemcpyDeviceToHost));
        LFQ_TRY_HIP(hipMemcpy(off.data(), T.off, (size_t)nl * LFQ_VC_NOFF * 2, hipMemcpyDeviceToHost));
        if (nr > 0) {
            LFQ_TRY_HIP(hipMemcpy(v->h_run_id.data(), T.run_id, (size_t)nr * 4, hipMemcpyDeviceToHost));
            if (T.rec_line) {
                LFQ_TRY_HIP(hipMemcpy(v->h_line.data(), T.rec_line, (size_t)nr * 8, hipMemcpyDeviceToHost));
            }
        }
        v->h_pos.resize((size_t)nr);
        v->h_qual.resize((size_t)nr);
        v->h_nf.resize((size_t)nr);
        v->h_flags.resize((size_t)nr);
        v->h_off.resize((size_t)nr * LFQ_VC_NOFF);
        for (int64_t r = 0; r < nr; r++) {
            const int64_t k = T.rec_line ? v->h_line[(size_t)r] : T.first + r;
            v->h_line[(size_t)r] = k;
            v->h_pos[(size_t)r] = pos[(size_t)k];
            v->h_qual[(size_t)r] = qual[(size_t)k];
            v->h_nf[(size_t)r] = nf[(size_t)k];
            v->h_flags[(size_t)r] = flags[(size_t)k];
            std::copy(off.begin() + (size_t)k * LFQ_VC_NOFF, off.begin() + (size_t)(k + 1) * LFQ_VC_NOFF, v->h_off.begin() + (size_t)r * LFQ_VC_NOFF);
        }
    }
    v->h_names.clear();
    for (const std::string &s : v->run_name) {
        v->h_names.push_back(s.c_str());
    }
    v->have_table = true;
    return LFQ_OK;
}

extern "C" {

void lfq_vcf_close(lfq_vcf *v)
{
    if (!v) {
        return;
    }
    (void)hipSetDevice(v->c->device);
    if (v->d_text) (void)hipFree(v->d_text);
    if (v->d_tab) (void)hipFree(v->d_tab);
    if (v->d_rec) (void)hipFree(v->d_rec);
    delete v;
}

int lfq_vcf_open(lfq_ctx *c, const uint8_t *bytes, int64_t n, int mode, lfq_vcf **out, int *why_out, int64_t *bad_line_out)
{
    if (why_out) *why_out = LFQ_VC_OK;
    if (bad_line_out) *bad_line_out = 0;
    if (!c || !out || n < 0 || (n > 0 && !bytes) || (mode != LFQ_VC_STREAM && mode != LFQ_VC_TABIX)) {
        return LFQ_ERR_INVALID;
    }
    *out = nullptr;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LfqVcfState *S = vc_state(c);
    memset(&S->times, 0, sizeof(S->times));
    S->scan_on = S->parse_on = S->info_on = S->match_on = S->emit_on = false;
    lfq_vcf *v = new lfq_vcf();
    v->c = c;
    v->mode = mode;
    memset(&v->D, 0, sizeof(v->D));
    v->d_text = v->d_tab = v->d_rec = nullptr;
    v->hdr_line = -1;
    v->lines_behind = 0;
    v->have_table = v->have_text = false;
    v->run_beg.assign(1, 0);
    LfqVcDev &D = v->D;
    D.T.n = n;
    D.n_chunks = (n + LFQ_VCF_CHUNK - 1) / LFQ_VCF_CHUNK;
    D.n_tiles = (D.n_chunks + LFQ_VCF_THREADS - 1) / LFQ_VCF_THREADS;
    S->times.n_bytes = n;
    if (n == 0) {
        *out = v;
        return LFQ_OK;
    }
    hipStream_t st = c->stream;
    auto fail = [&](int why) {
        (void)hipStreamSynchronize(st);
        lfq_vcf_close(v);
        return why;
    };
    const int64_t padded = D.n_chunks * LFQ_VCF_CHUNK + 16, o_tn = lfq_al(padded), o_atom = o_tn + lfq_al((D.n_tiles + 1) * 8),
                  total = o_atom + lfq_al(3 * 8);
    if (hipMalloc((void **)&v->d_text, (size_t)total) != hipSuccess) {
        v->d_text = nullptr;
        return fail(LFQ_ERR_NOMEM);
    }
    D.T.text = v->d_text;
    D.tile_nl = (int64_t *)(v->d_text + o_tn);
    D.atom = (unsigned long long *)(v->d_text + o_atom);
    /* the file: from the context's live inflate result when it lies there (a bgzip-compressed VCF), else across the link */
    const double t0 = lfq_now_ms();
    const uint8_t *res = lfq_bgzf_resident_bytes(c, bytes, n);
    const int64_t tail = n / LFQ_VCF_CHUNK * LFQ_VCF_CHUNK;
    if (hipMemsetAsync(v->d_text + tail, 0, (size_t)(padded - tail), st) != hipSuccess
        || hipMemsetAsync(D.atom, 0xff, 3 * 8, st) != hipSuccess
        || hipMemcpyAsync(v->d_text, res ? res : bytes, (size_t)n, res ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st) != hipSuccess
        || hipStreamSynchronize(st) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    S->times.upload_ms = lfq_now_ms() - t0;
    S->times.n_from_device = res ? 1 : 0;
    int rc = LFQ_OK;
    if ((rc = S->scan_t.begin(st)) != LFQ_OK) {
        return fail(rc);
    }
    hipLaunchKernelGGL(lfq_vcf_tiles_kernel, dim3((unsigned)D.n_tiles), dim3(LFQ_VCF_THREADS), 0, st, D);
    hipLaunchKernelGGL(lfq_vcf_sums_kernel, dim3(1), dim3(LFQ_VCF_SCAN_LANES), 0, st, D);
    int64_t n_starts = 0;
    if (!vc_launched() || hipMemcpyAsync(&n_starts, D.tile_nl + D.n_tiles, 8, hipMemcpyDeviceToHost, st) != hipSuccess
        || hipStreamSynchronize(st) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    const int64_t nl = 1 + n_starts;
    D.T.n_lines = nl;
    const int64_t o_pos = lfq_al((nl + 1) * 8), o_ex = o_pos + lfq_al(nl * 8), o_qual = o_ex + lfq_al((nl + 1) * 8), o_val = o_qual + lfq_al(nl * 4),
                  o_off = o_val + lfq_al(nl * 4), o_nf = o_off + lfq_al(nl * LFQ_VC_NOFF * 2), o_fl = o_nf + lfq_al(nl), tab_total = o_fl + lfq_al(nl);
    if (hipMalloc((void **)&v->d_tab, (size_t)tab_total) != hipSuccess) {
        v->d_tab = nullptr;
        return fail(LFQ_ERR_NOMEM);
    }
    D.lstart = (int64_t *)v->d_tab;
    D.pos = (int64_t *)(v->d_tab + o_pos);
    D.ex = (int64_t *)(v->d_tab + o_ex);
    D.qual = (int32_t *)(v->d_tab + o_qual);
    D.val = (int32_t *)(v->d_tab + o_val);
    D.off = (uint16_t *)(v->d_tab + o_off);
    D.nf = v->d_tab + o_nf;
    D.flags = v->d_tab + o_fl;
    D.T.lstart = D.lstart; D.T.pos = D.pos; D.T.qual = D.qual; D.T.off = D.off; D.T.nf = D.nf; D.T.flags = D.flags;
    hipLaunchKernelGGL(lfq_vcf_emit_kernel, dim3((unsigned)D.n_tiles), dim3(LFQ_VCF_THREADS), 0, st, D, mode);
    if (!vc_launched() || S->scan_t.end(st) != LFQ_OK || S->parse_t.begin(st) != LFQ_OK) {
        return fail(LFQ_ERR_HIP);
    }
    S->scan_on = true;
    hipLaunchKernelGGL(lfq_vcf_parse_kernel, dim3(vc_grid(nl)), dim3(256), 0, st, D, mode);
    S->times.n_launches = 4;
    if (!vc_launched()) {
        return fail(LFQ_ERR_HIP);
    }
    int64_t nr = 0;
    if (mode == LFQ_VC_STREAM) {
        unsigned long long at[2] = {VC_NONE, VC_NONE};
        if (hipMemcpyAsync(at, D.atom, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            return fail(LFQ_ERR_HIP);
        }
        v->hdr_line = at[0] == VC_NONE ? -1 : (int64_t)at[0];
        D.T.first = v->hdr_line + 1;
        const int64_t end = at[1] == VC_NONE ? nl : (int64_t)at[1];
        nr = end - D.T.first;
        v->lines_behind = nl - end;
        if (v->hdr_line >= 0) {
            int64_t at_byte = 0;
            for (int64_t k = 0; k <= v->hdr_line && at_byte < n; k++) {         /* the header: the caller's bytes up to that line's end */
                const void *p = memchr(bytes + at_byte, '\n', (size_t)(n - at_byte));
                at_byte = p ? (const uint8_t *)p - bytes + 1 : n;
            }
            v->header.assign((const char *)bytes, (size_t)at_byte);
        }
    } else {
        if ((rc = vc_exscan(v, nl, &nr, S)) != LFQ_OK) {
            return fail(rc);
        }
    }
    D.T.n_rec = nr;
    const int64_t nr1 = std::max<int64_t>(nr, 1), o_rid = lfq_al(nr1 * 8), o_rb = o_rid + lfq_al(nr1 * 4), o_hd = o_rb + lfq_al((nr1 + 1) * 8),
                  rec_total = o_hd + lfq_al(nr1 * (int64_t)sizeof(LfqVcHead));
    if (hipMalloc((void **)&v->d_rec, (size_t)rec_total) != hipSuccess) {
        v->d_rec = nullptr;
        return fail(LFQ_ERR_NOMEM);
    }
    int64_t *d_rec_line = (int64_t *)v->d_rec, *d_run_beg = (int64_t *)(v->d_rec + o_rb);
    int32_t *d_run_id = (int32_t *)(v->d_rec + o_rid);
    LfqVcHead *d_heads = (LfqVcHead *)(v->d_rec + o_hd);
    std::vector<LfqVcHead> heads;
    int64_t n_runs = 0;
    if (mode == LFQ_VC_TABIX && nr > 0) {
        hipLaunchKernelGGL(lfq_vcf_scatter_kernel, dim3(vc_grid(nl)), dim3(256), 0, st, D.val, D.ex, nl, d_rec_line, (int32_t *)nullptr);
        S->times.n_launches += 1;
        D.T.rec_line = d_rec_line;
    }
    if (nr > 0) {
        hipLaunchKernelGGL(lfq_vcf_runs_kernel, dim3(vc_grid(nr)), dim3(256), 0, st, D, mode);
        S->times.n_launches += 1;
        if ((rc = vc_exscan(v, nr, &n_runs, S)) != LFQ_OK) {
            return fail(rc);
        }
        hipLaunchKernelGGL(lfq_vcf_scatter_kernel, dim3(vc_grid(nr)), dim3(256), 0, st, D.val, D.ex, nr, d_run_beg, d_run_id);
        D.T.run_id = d_run_id;
        D.T.run_beg = d_run_beg;
        D.T.n_runs = n_runs;
        hipLaunchKernelGGL(lfq_vcf_heads_kernel, dim3(vc_grid(n_runs)), dim3(256), 0, st, D, d_heads);
        S->times.n_launches += 2;
        heads.resize((size_t)n_runs);
        if (!vc_launched() || hipMemcpyAsync(d_run_beg + n_runs, &D.T.n_rec, 8, hipMemcpyHostToDevice, st) != hipSuccess
            || hipMemcpyAsync(heads.data(), d_heads, (size_t)n_runs * sizeof(LfqVcHead), hipMemcpyDeviceToHost, st) != hipSuccess) {
            return fail(LFQ_ERR_HIP);
        }
    } else {
        D.T.run_beg = d_run_beg;
        D.T.run_id = d_run_id;
        if (hipMemsetAsync(d_run_beg, 0, 8, st) != hipSuccess) {
            return fail(LFQ_ERR_HIP);
        }
    }
    unsigned long long bad = VC_NONE;
    if (S->parse_t.end(st) != LFQ_OK || hipMemcpyAsync(&bad, D.atom + 2, 8, hipMemcpyDeviceToHost, st) != hipSuccess
        || hipStreamSynchronize(st) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    S->parse_on = true;
    S->times.n_lines = nl;
    S->times.n_records = nr;
    v->run_beg.clear();
    for (const LfqVcHead &h : heads) {
        v->run_name.emplace_back((const char *)bytes + h.name_beg, (size_t)h.name_len);
    }
    if (n_runs > 0) {
        v->run_beg.resize((size_t)n_runs + 1);
        if (hipMemcpy(v->run_beg.data(), d_run_beg, (size_t)(n_runs + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            return fail(LFQ_ERR_HIP);
        }
    } else {
        v->run_beg.assign(1, 0);
    }
    if (mode == LFQ_VC_TABIX && bad == VC_NONE) {       /* one run per name: few names, on the host */
        for (size_t i = 0; i < v->run_name.size(); i++) {
            for (size_t j = 0; j < i; j++) {
                if (v->run_name[i] == v->run_name[j]) {
                    bad = std::min(bad, (unsigned long long)heads[i].line * 8ull + LFQ_VC_UNSORTED);
                }
            }
        }
    }
    if (bad != VC_NONE) {
        /* the refusal comes from the smallest (line, why) alone: whatever order the lanes ran in */
        if (why_out) *why_out = (int)(bad % 8);
        if (bad_line_out) *bad_line_out = (int64_t)(bad / 8) + 1;
        return fail(LFQ_ERR_INVALID);
    }
    *out = v;
    return LFQ_OK;
}

int64_t lfq_vcf_n_records(const lfq_vcf *v) { return v ? v->D.T.n_rec : 0; }
int64_t lfq_vcf_n_lines_behind(const lfq_vcf *v) { return v ? v->lines_behind : 0; }

int lfq_vcf_header(lfq_vcf *v, const char **text, int64_t *n, int *found)
{
    if (!v || !text || !n || !found) {
        return LFQ_ERR_INVALID;
    }
    *text = v->header.c_str();
    *n = (int64_t)v->header.size();
    *found = v->hdr_line >= 0 ? 1 : 0;
    return LFQ_OK;
}

int lfq_vcf_records(lfq_vcf *v, lfq_vcf_table *out)
{
    if (!v || !out) {
        return LFQ_ERR_INVALID;
    }
    LFQ_TRY(vc_host_table(v));
    out->n_records = v->D.T.n_rec;
    out->n_lines = v->D.T.n_lines;
    out->n_runs = (int64_t)v->run_name.size();
    out->line = v->h_line.data();
    out->line_start = v->h_lstart.data();
    out->pos = v->h_pos.data();
    out->qual = v->h_qual.data();
    out->flags = v->h_flags.data();
    out->n_fields = v->h_nf.data();
    out->field_off = v->h_off.data();
    out->run_id = v->h_run_id.data();
    out->run_begin = v->run_beg.data();
    out->run_name = v->h_names.data();
    return LFQ_OK;
}

/* the INFO values of every record, on the host */
static int vc_info(lfq_vcf *v, std::vector<LfqVcInfo> *info)
{
    const int64_t nr = v->D.T.n_rec;
    info->resize((size_t)nr);
    if (nr == 0) {
        return LFQ_OK;
    }
    lfq_ctx *c = v->c;
    LfqVcfState *S = vc_state(c);
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    LfqVcInfo *d = nullptr;
    if (hipMalloc((void **)&d, (size_t)nr * sizeof(LfqVcInfo)) != hipSuccess) {
        return LFQ_ERR_NOMEM;
    }
    int rc = S->info_t.begin(st);
    if (rc == LFQ_OK) {
        hipLaunchKernelGGL(lfq_vcf_info_kernel, dim3(vc_grid(nr)), dim3(256), 0, st, v->D.T, d);
        S->times.n_launches += 1;
        if (!vc_launched() || S->info_t.end(st) != LFQ_OK
            || hipMemcpyAsync(info->data(), d, (size_t)nr * sizeof(LfqVcInfo), hipMemcpyDeviceToHost, st) != hipSuccess
            || hipStreamSynchronize(st) != hipSuccess) {
            rc = LFQ_ERR_HIP;
        } else {
            S->info_on = true;
        }
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    return rc;
}

/* strtof on the bytes the device found: the C library's own, so that af is the reference's bit for bit */
static float vc_af(const lfq_vcf *v, const LfqVcInfo &I)
{
    const std::string s((const char *)v->h_text.data() + I.af_beg, (size_t)I.af_len);
    return strtof(s.c_str(), nullptr);
}

int lfq_vcf_filter_vars(lfq_vcf *v, lfq_filter_var *out)
{
    if (!v || (v->D.T.n_rec > 0 && !out)) {
        return LFQ_ERR_INVALID;
    }
    std::vector<LfqVcInfo> info;
    LFQ_TRY(vc_info(v, &info));
    LFQ_TRY(vc_host_table(v));
    LFQ_TRY(vc_host_text(v));
    for (int64_t r = 0; r < v->D.T.n_rec; r++) {
        const LfqVcInfo &I = info[(size_t)r];
        lfq_filter_var &x = out[r];
        x.is_indel = lfq_vc_is_indel(v->h_flags[(size_t)r]) ? 1 : 0;
        x.qual = v->h_qual[(size_t)r];
        x.dp = I.dp;
        x.sb = I.sb;
        x.alt_fw = I.dp4[2];
        x.alt_rv = I.dp4[3];
        x.af = (I.has & 8) ? vc_af(v, I) : 0.f;
        x.pad_ = 0;
    }
    return LFQ_OK;
}

int lfq_vcf_uniq_variants(lfq_vcf *v, const char *chrom, int only_unfiltered, float uni_freq, lfq_uniq_variants *out,
                          int64_t **line_of_variant, int64_t *bad_line_out)
{
    if (bad_line_out) *bad_line_out = 0;
    if (!v || !chrom || !out || !line_of_variant) {
        return LFQ_ERR_INVALID;
    }
    std::vector<LfqVcInfo> info;
    LFQ_TRY(vc_info(v, &info));
    LFQ_TRY(vc_host_table(v));
    LFQ_TRY(vc_host_text(v));
    v->u_pos.clear(); v->u_line.clear(); v->u_key.clear(); v->u_af.clear(); v->u_ref.clear(); v->u_alt.clear();
    v->u_ref_off.assign(1, 0);
    v->u_alt_off.assign(1, 0);
    for (int64_t r = 0; r < v->D.T.n_rec; r++) {
        const uint8_t fl = v->h_flags[(size_t)r];
        if (v->run_name[(size_t)v->h_run_id[(size_t)r]] != chrom || (only_unfiltered && (fl & LFQ_VC_F_FILTERED))) {
            continue;
        }
        const LfqVcInfo &I = info[(size_t)r];
        if (!(uni_freq > 0.f) && !(I.has & 8)) {
            if (bad_line_out) *bad_line_out = v->h_line[(size_t)r] + 1;
            return LFQ_ERR_INVALID;
        }
        const uint16_t *off = v->h_off.data() + (size_t)r * LFQ_VC_NOFF;
        const char *line = (const char *)v->h_text.data() + v->h_lstart[(size_t)v->h_line[(size_t)r]];
        v->u_ref.append(line + lfq_vc_fbeg(off, 3), (size_t)(lfq_vc_fend(off, 3) - lfq_vc_fbeg(off, 3)));
        v->u_alt.append(line + lfq_vc_fbeg(off, 4), (size_t)(lfq_vc_fend(off, 4) - lfq_vc_fbeg(off, 4)));
        v->u_ref_off.push_back((int64_t)v->u_ref.size());
        v->u_alt_off.push_back((int64_t)v->u_alt.size());
        v->u_pos.push_back(v->h_pos[(size_t)r]);
        v->u_line.push_back(v->h_line[(size_t)r]);
        v->u_key.push_back((fl & LFQ_VC_F_INDEL_KEY) ? 1 : 0);
        v->u_af.push_back(uni_freq > 0.f ? uni_freq : vc_af(v, I));
    }
    out->n = (int64_t)v->u_pos.size();
    out->pos = v->u_pos.data();
    out->ref_off = v->u_ref_off.data();
    out->alt_off = v->u_alt_off.data();
    out->ref = v->u_ref.c_str();
    out->alt = v->u_alt.c_str();
    out->indel_key_or_null = v->u_key.data();
    out->af = v->u_af.data();
    *line_of_variant = v->u_line.data();
    return LFQ_OK;
}

int lfq_vcf_ign_mask(lfq_vcf *v, const char *chrom, int64_t ref_len, const lfq_bed *bed, uint8_t *mask)
{
    if (!v || !chrom || ref_len < 0 || (ref_len > 0 && !mask)) {
        return LFQ_ERR_INVALID;
    }
    bool any = false;
    for (const std::string &s : v->run_name) {
        any = any || s == chrom;
    }
    if (!any || ref_len == 0) {
        return LFQ_OK;
    }
    lfq_ctx *c = v->c;
    LfqVcfState *S = vc_state(c);
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    LfqBedTab tab = {nullptr, nullptr, -1};
    const LfqBedName *bn = bed ? bed->find(chrom) : nullptr;
    const int64_t nb = bn ? (int64_t)bn->beg.size() : 0, o_beg = lfq_al(ref_len), o_pmax = o_beg + lfq_al(std::max<int64_t>(nb, 1) * 4),
                  total = o_pmax + lfq_al(std::max<int64_t>(nb, 1) * 4);
    uint8_t *d = nullptr;
    if (hipMalloc((void **)&d, (size_t)total) != hipSuccess) {
        return LFQ_ERR_NOMEM;
    }
    int rc = LFQ_OK;
    std::vector<uint8_t> got((size_t)ref_len);
    if (bed) {
        tab.beg = (const int32_t *)(d + o_beg);
        tab.pmax = (const int32_t *)(d + o_pmax);
        tab.n = nb;                     /* a name the BED lacks: an empty table, nothing overlaps */
        if (nb > 0 && (hipMemcpyAsync(d + o_beg, bn->beg.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st) != hipSuccess
                       || hipMemcpyAsync(d + o_pmax, bn->pmax.data(), (size_t)nb * 4, hipMemcpyHostToDevice, st) != hipSuccess)) {
            rc = LFQ_ERR_HIP;
        }
    }
    if (rc == LFQ_OK && hipMemsetAsync(d, 0, (size_t)ref_len, st) != hipSuccess) {
        rc = LFQ_ERR_HIP;
    }
    for (size_t h = 0; rc == LFQ_OK && h < v->run_name.size(); h++) {
        if (v->run_name[h] == chrom) {
            const int64_t r0 = v->run_beg[h], r1 = v->run_beg[h + 1];
            hipLaunchKernelGGL(lfq_vcf_mask_kernel, dim3(vc_grid(r1 - r0)), dim3(256), 0, st, v->D.T, r0, r1, ref_len, tab, d);
            S->times.n_launches += 1;
        }
    }
    if (rc == LFQ_OK && (!vc_launched() || hipMemcpyAsync(got.data(), d, (size_t)ref_len, hipMemcpyDeviceToHost, st) != hipSuccess)) {
        rc = LFQ_ERR_HIP;
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == LFQ_OK) {
        rc = LFQ_ERR_HIP;
    }
    (void)hipFree(d);
    LFQ_TRY(rc);
    for (int64_t i = 0; i < ref_len; i++) {
        mask[i] |= got[(size_t)i];
    }
    return LFQ_OK;
}

int lfq_vcfset(lfq_vcf *one, lfq_vcf *two, lfq_vcf *const *more, int64_t n_more, const lfq_vcfset_conf *conf, const lfq_vcfset_result **out)
{
    if (!one || !conf || !out || n_more < 0 || (n_more > 0 && !more) || conf->op < LFQ_VC_OP_INTERSECT || conf->op > LFQ_VC_OP_CONCAT
        || (conf->only_snvs && conf->only_indels) || (conf->op != LFQ_VC_OP_CONCAT && (!two || n_more > 0))) {
        return LFQ_ERR_INVALID;
    }
    for (int64_t i = 0; i < n_more; i++) {
        if (!more[i] || more[i]->c != one->c) {
            return LFQ_ERR_INVALID;
        }
    }
    if (conf->op != LFQ_VC_OP_CONCAT && two->c != one->c) {
        return LFQ_ERR_INVALID;
    }
    *out = nullptr;
    lfq_ctx *c = one->c;
    LfqVcfState *S = vc_state(c);
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    S->match_on = S->emit_on = false;
    S->times.match_ms = S->times.emit_ms = S->times.download_ms = 0.0;
    const int launches0 = S->times.n_launches;
    std::vector<lfq_vcf *> files(1, one);
    if (conf->op == LFQ_VC_OP_CONCAT) {
        files.insert(files.end(), more, more + n_more);
    }
    LfqVcSetConf sc = {conf->op, conf->only_passed, conf->only_pos, conf->only_snvs, conf->only_indels};
    const std::string add = conf->add_info_or_null ? conf->add_info_or_null : "";
    int64_t n_keep = 0, max_runs = 1;
    for (lfq_vcf *f : files) {
        n_keep += f->D.T.n_rec;
        max_runs = std::max<int64_t>(max_runs, (int64_t)f->run_name.size());
    }
    lfq_vcfset_result &R = S->res;
    memset(&R, 0, sizeof(R));
    S->keep.assign((size_t)n_keep, 0);
    const int64_t o_cnt = lfq_al(std::max<int64_t>(n_keep, 1)), o_map = o_cnt + lfq_al(4 * 8), o_add = o_map + lfq_al(max_runs * 8),
                  total = o_add + lfq_al((int64_t)add.size() + 16);
    LFQ_TRY(grow(&S->d_work, &S->d_work_cap, total));
    uint8_t *d = S->d_work, *d_out = nullptr;
    uint8_t *d_keep = d;
    unsigned long long *d_cnt = (unsigned long long *)(d + o_cnt), cnt[4] = {0, 0, 0, VC_NONE};
    int64_t *d_map = (int64_t *)(d + o_map);
    char *d_add = (char *)(d + o_add);
    int rc = LFQ_OK;
    std::vector<int64_t> bases(files.size() + 1, 0);
    int64_t at = 0;
    if (hipMemcpyAsync(d_cnt, cnt, 32, hipMemcpyHostToDevice, st) != hipSuccess
        || (!add.empty() && hipMemcpyAsync(d_add, add.data(), add.size(), hipMemcpyHostToDevice, st) != hipSuccess)
        || S->match_t.begin(st) != LFQ_OK) {
        rc = LFQ_ERR_HIP;
        goto done;
    }
    for (size_t f = 0; f < files.size(); f++) {
        lfq_vcf *A = files[f];
        if (A->D.T.n_rec > 0) {
            const LfqVcTab &TB = conf->op == LFQ_VC_OP_CONCAT ? A->D.T : two->D.T;
            if (conf->op != LFQ_VC_OP_CONCAT) {
                const std::vector<int64_t> map = lfq_vc_run_map(A->run_name, two->run_name);
                if (hipMemcpyAsync(d_map, map.data(), map.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess
                    || hipStreamSynchronize(st) != hipSuccess) {
                    rc = LFQ_ERR_HIP;
                    goto done;
                }
            }
            hipLaunchKernelGGL(lfq_vcf_match_kernel, dim3(vc_grid(A->D.T.n_rec)), dim3(256), 0, st, A->D.T, TB, d_map, sc, (int)f, d_keep + at,
                               d_cnt, d_cnt + 3);
            S->times.n_launches += 1;
        }
        at += A->D.T.n_rec;
    }
    if (!vc_launched() || S->match_t.end(st) != LFQ_OK || hipMemcpyAsync(cnt, d_cnt, 32, hipMemcpyDeviceToHost, st) != hipSuccess
        || (n_keep > 0 && hipMemcpyAsync(S->keep.data(), d_keep, (size_t)n_keep, hipMemcpyDeviceToHost, st) != hipSuccess)
        || hipStreamSynchronize(st) != hipSuccess) {
        rc = LFQ_ERR_HIP;
        goto done;
    }
    S->match_on = true;
    if (cnt[3] != VC_NONE) {
        R.why = (int)(cnt[3] % 8);
        R.bad_file = (int)((cnt[3] / 8) >> 40);
        R.bad_line = (int64_t)((cnt[3] / 8) & ((1ull << 40) - 1)) + 1;
        S->keep.clear();
        *out = &R;
        rc = LFQ_ERR_INVALID;
        goto done;
    }
    R.n_vars1 = (int64_t)cnt[0];
    R.n_ignored = (int64_t)cnt[1];
    R.n_out = (int64_t)cnt[2];
    R.n_keep = n_keep;
    R.keep = S->keep.data();
    if (!conf->count_only) {
        /* plan: the written length of every record, offsets by scan; file f's lines start at bases[f] */
        const int64_t hdr = one->hdr_line >= 0 ? (int64_t)one->header.size() : 0;
        bases[0] = hdr;
        at = 0;
        if (S->emit_t.begin(st) != LFQ_OK) {
            rc = LFQ_ERR_HIP;
            goto done;
        }
        for (size_t f = 0; f < files.size(); f++) {
            lfq_vcf *A = files[f];
            int64_t len = 0;
            if (A->D.T.n_rec > 0 && R.n_out > 0) {
                hipLaunchKernelGGL(lfq_vcf_plan_kernel, dim3(vc_grid(A->D.T.n_rec)), dim3(256), 0, st, A->D.T, d_keep + at, (int)add.size(), A->D.val);
                S->times.n_launches += 1;
                if ((rc = vc_exscan(A, A->D.T.n_rec, &len, S)) != LFQ_OK) {
                    goto done;
                }
            }
            bases[f + 1] = bases[f] + len;
            at += A->D.T.n_rec;
        }
        const int64_t n_text = bases.back();
        if (grow_pinned(&S->h_text, &S->h_text_cap, n_text + 1) != LFQ_OK
            || grow(&S->d_out, &S->d_out_cap, (n_text + 15) / 16 * 16 + 16) != LFQ_OK) {
            rc = LFQ_ERR_NOMEM;
            goto done;
        }
        d_out = S->d_out;
        if (hdr > 0 && hipMemcpyAsync(d_out, one->d_text, (size_t)hdr, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            rc = LFQ_ERR_HIP;
            goto done;
        }
        for (size_t f = 0; f < files.size(); f++) {
            const int64_t len = bases[f + 1] - bases[f];
            if (len > 0) {
                const int64_t chunks = (bases[f + 1] + 15) / 16 - bases[f] / 16;
                hipLaunchKernelGGL(lfq_vcf_copy_kernel, dim3(vc_grid(chunks)), dim3(256), 0, st, files[f]->D.T, files[f]->D.ex, bases[f], d_add,
                                   (int)add.size(), d_out);
                S->times.n_launches += 1;
            }
        }
        if (!vc_launched() || S->emit_t.end(st) != LFQ_OK || hipStreamSynchronize(st) != hipSuccess) {
            rc = LFQ_ERR_HIP;
            goto done;
        }
        S->emit_on = true;
        const double t0 = lfq_now_ms();
        if (n_text > 0 && (hipMemcpyAsync(S->h_text, d_out, (size_t)n_text, hipMemcpyDeviceToHost, st) != hipSuccess
                           || hipStreamSynchronize(st) != hipSuccess)) {
            rc = LFQ_ERR_HIP;
            goto done;
        }
        S->times.download_ms = lfq_now_ms() - t0;
        S->h_text[n_text] = 0;
        R.text = (const char *)S->h_text;
        R.text_bytes = n_text;
    }
    S->times.n_set_launches = S->times.n_launches - launches0;
    *out = &R;
done:
    (void)hipStreamSynchronize(st);
    return rc;
}

int lfq_last_vcf_times(lfq_ctx *c, lfq_vcf_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    LfqVcfState *S = vc_state(c);
    if (S->scan_on) LFQ_TRY(S->scan_t.ms(&S->times.scan_ms));
    if (S->parse_on) LFQ_TRY(S->parse_t.ms(&S->times.parse_ms));
    if (S->info_on) LFQ_TRY(S->info_t.ms(&S->times.info_ms));
    if (S->match_on) LFQ_TRY(S->match_t.ms(&S->times.match_ms));
    if (S->emit_on) LFQ_TRY(S->emit_t.ms(&S->times.emit_ms));
    *t = S->times;
    return LFQ_OK;
}

}
