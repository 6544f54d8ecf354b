/*
 * lfq_indelqual.hip -- `lofreq indelqual` (lofreq_indelqual.c:42-215): the BI / BD per-base indel qualities of a batch of
 * reads of one contig, written where the indel pileup reads them.
 *
 * Dindel mode (dindel_fetch_func, :136-215): a base aligned to reference position x by an M / = / X operation gets
 * DINDELQ[hpcount[x + 1]] (:180-181), where find_homopolymers (:109-133) gave hpcount the run length at the FIRST base of a
 * homopolymer run and 1 everywhere else; '!' past rlen - 2 and for a count above 18.  Every base of an I / S operation gets '!'
 * (:188-193).  That value depends on x alone:
 *     x > rlen - 2                     -> '!'
 *     ref[x + 1] == ref[x]             -> 'M'   (x + 1 is not the first base of its run: count 1; upper-cased, :155)
 *     else L = run starting at x + 1   -> L > 18 ? '!' : DINDELQ[L]
 * so the work is two kernels:
 *   table  one byte per reference position the batch covers.  A workgroup of 256 threads takes 4096 positions: the contig bytes
 *          of the tile and a halo behind it go to LDS once (upper-cased, 16 bytes per lane), a lane reads the 48 bytes around
 *          its 16 positions back as three 16-byte LDS reads, gets the run lengths by one backward pass in registers and stores 16
 *          table bytes.  The halo is 19 bytes of look-ahead -- position x needs the run that starts at x + 1 up to length 19.
 *   fill   the output is taken as what it is in memory, a flat array of n_bases bytes: a lane owns 16 consecutive ALIGNED bytes
 *          and stores them as one 16-byte word (a wavefront: 1 KiB contiguous per store instruction), whichever reads they
 *          belong to.  It finds the read of its first byte by binary search in seq_off, walks that read's CIGAR to the byte
 *          and from there on, into the next reads where the 16 bytes cross a boundary.  A lane per read or a wavefront per
 *          read would have to store single bytes: reads start at arbitrary byte offsets of the seq_off layout.  The search
 *          reads the same few cache lines in every lane of a wavefront; the CIGAR walk is a handful of operations.
 * Uniform mode (:69-104, 218-258) is the fill kernel with two constants and no search.
 * In Dindel mode BI and BD are the same string (:205, 211): one array is written and both pointers name it.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lfq_internal.h"

#define LFQ_IDQ_TILE 4096                   /* table positions per workgroup: 256 lanes x 16 */
#define LFQ_IDQ_HALO 32                     /* bytes staged behind a tile (19 are needed; 32 keeps the staging in 16-byte words) */

/* char DINDELQ[] = "!MMMLKEC@=<;:988776" (lofreq_indelqual.c:42), indexed by the homopolymer count */
__host__ __device__ static inline uint8_t lfq_idq_dindelq(int count)
{
    return (uint8_t)(count > 18 ? '!' : "!MMMLKEC@=<;:988776"[count]);
}

__host__ __device__ static inline uint8_t lfq_idq_upper(uint8_t ch)
{
    return (uint8_t)((ch >= 'a' && ch <= 'z') ? ch - 32 : ch);
}

/* the table byte of reference position x, straight from the contig: what the host needs for the one base of an indel event */
uint8_t lfq_idq_ref_byte(const char *ref, int64_t ref_len, int64_t x)
{
    if (x < 0 || x > ref_len - 2) {
        return '!';
    }
    const uint8_t a = lfq_idq_upper((uint8_t)ref[x]), b = lfq_idq_upper((uint8_t)ref[x + 1]);
    if (a == b) {
        return 'M';
    }
    int run = 1;
    while (run < 19 && x + 1 + run < ref_len && lfq_idq_upper((uint8_t)ref[x + 1 + run]) == b) {
        run++;
    }
    return lfq_idq_dindelq(run);
}

/* the Dindel byte of query base qpos of one read (host): the CIGAR walk of dindel_fetch_func up to that base */
uint8_t lfq_idq_host_byte(const char *ref, int64_t ref_len, int64_t pos, const uint32_t *cigar, int n_cigar, int64_t qpos)
{
    int64_t x = pos, y = 0;
    for (int k = 0; k < n_cigar; k++) {
        const int op = (int)(cigar[k] & 0xf);
        const int64_t len = cigar[k] >> 4;
        if (op == 0 || op == 7 || op == 8) {
            if (qpos < y + len) {
                return lfq_idq_ref_byte(ref, ref_len, x + (qpos - y));
            }
            x += len;
            y += len;
        } else if (op == 1 || op == 4) {
            if (qpos < y + len) {
                return '!';
            }
            y += len;
        } else if (op == 2) {
            x += len;
        }
    }
    return '!';
}

/* tab[x - tab_begin] for x in [tab_begin, tab_end): tab_begin is a multiple of 16, tab_end <= ref_len */
__global__ __launch_bounds__(256) void lfq_idq_table_kernel(const uint8_t *__restrict__ ref, int64_t ref_len, int64_t tab_begin,
                                                            int64_t tab_end, uint8_t *__restrict__ tab)
{
    __shared__ uint4 s_tile[(LFQ_IDQ_TILE + LFQ_IDQ_HALO) / 16];
    const int t = (int)threadIdx.x;
    const int64_t tile0 = tab_begin + (int64_t)blockIdx.x * LFQ_IDQ_TILE;
    /* stage: 258 words of 16 upper-cased contig bytes; a byte at or past ref_len is 0 and never looked at as a letter */
    for (int w = t; w < (LFQ_IDQ_TILE + LFQ_IDQ_HALO) / 16; w += 256) {
        const int64_t g = tile0 + (int64_t)w * 16;
        uint32_t v[4] = {0, 0, 0, 0};
        if (g + 16 <= ref_len && ((uintptr_t)(ref + g) & 15) == 0) {
            const uint4 q = *(const uint4 *)(ref + g);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int j = 0; j < 16; j++) {
                const uint32_t b = g + j < ref_len ? ref[g + j] : 0u;
                v[j >> 2] |= b << (8 * (j & 3));
            }
        }
        for (int j = 0; j < 4; j++) {           /* four letters at a time: bytes in 'a'..'z' lose bit 5 */
            const uint32_t x = v[j], lo = (x & 0x7f7f7f7fu) + 0x1f1f1f1fu, hi = (x & 0x7f7f7f7fu) + 0x05050505u;
            v[j] = x ^ ((lo & ~hi & ~x & 0x80808080u) >> 2);
        }
        s_tile[w] = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    const int64_t x0 = tile0 + (int64_t)t * 16;
    if (x0 >= tab_end) {
        return;
    }
    /* letters x0 .. x0 + 47 of which x0 .. x0 + 35 are used */
    uint32_t w[12];
    for (int j = 0; j < 3; j++) {
        const uint4 q = s_tile[t + j];
        w[4 * j] = q.x; w[4 * j + 1] = q.y; w[4 * j + 2] = q.z; w[4 * j + 3] = q.w;
    }
    auto letter = [&](int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; };
    /* run[i] = length of the run of equal letters starting at x0 + i, cut at ref_len and saturating at 19: one backward pass.
     * Position x0 + 15 looks at the run from x0 + 16, exact up to 19 when the pass starts 19 letters further on, at x0 + 35. */
    uint32_t out[4] = {0, 0, 0, 0};
    int run = 1;                                /* of letter 35, as far as this lane can see */
#pragma unroll
    for (int i = 34; i >= 1; i--) {
        const bool same = letter(i) == letter(i + 1) && x0 + i + 1 < ref_len;
        run = same ? min(run + 1, 19) : 1;
        if (i <= 16) {                          /* run = that of position p = x0 + i: the answer for x = p - 1 */
            const int64_t x = x0 + i - 1;
            uint32_t b;
            if (x > ref_len - 2) {
                b = '!';
            } else if (letter(i - 1) == letter(i)) {
                b = 'M';
            } else {
                b = lfq_idq_dindelq(run);
            }
            out[(i - 1) >> 2] |= b << (8 * ((i - 1) & 3));
        }
    }
    *(uint4 *)(tab + (x0 - tab_begin)) = make_uint4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(256) void lfq_idq_fill_kernel(LfqIdqArgs A)
{
    const int64_t chunk = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t b0 = chunk * 16;
    if (b0 >= A.n_bases) {
        return;
    }
    if (A.tab == nullptr) {                     /* uniform: ENCODE_Q(ins_qual + 33) / ENCODE_Q(del_qual + 33) in every byte */
        const uint32_t wi = A.ins_byte * 0x01010101u, wd = A.del_byte * 0x01010101u;
        *(uint4 *)(A.bi_out + b0) = make_uint4(wi, wi, wi, wi);
        *(uint4 *)(A.bd_out + b0) = make_uint4(wd, wd, wd, wd);
        return;
    }
    /* the read of byte b0: the last r with seq_off[r] <= b0 (reads without bases in front of it are passed over) */
    int64_t lo = 0, hi = A.n_reads;             /* seq_off[lo] <= b0 < seq_off[hi] */
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (A.seq_off[mid] <= b0) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    int64_t r = lo;
    int64_t r_end = A.seq_off[r + 1];           /* first byte of the next read */
    int64_t k = A.cigar_off[r], k_end = A.cigar_off[r + 1];
    int64_t x = A.pos[r];
    int64_t left = 0;                           /* query bases left in the current operation */
    bool match = false;
    {
        int64_t skip = b0 - A.seq_off[r];       /* query bases of the read in front of byte b0 */
        while (k < k_end) {
            const uint32_t c = A.cigar[k++];
            const int op = (int)(c & 0xf);
            const int64_t len = c >> 4;
            if (op == 2) {
                x += len;
            } else if (op == 0 || op == 7 || op == 8 || op == 1 || op == 4) {
                match = op != 1 && op != 4;
                if (skip < len) {
                    left = len - skip;
                    x += match ? skip : 0;
                    break;
                }
                skip -= len;
                x += match ? len : 0;
            }
        }
    }
    uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int64_t b = b0 + i;
        uint32_t v = '!';
        if (b < A.n_bases) {
            while (b >= r_end && r + 1 < A.n_reads) {       /* on to the next read with bases */
                r++;
                r_end = A.seq_off[r + 1];
                k = A.cigar_off[r];
                k_end = A.cigar_off[r + 1];
                x = A.pos[r];
                left = 0;
            }
            while (left == 0 && k < k_end) {                /* on to the next operation with query bases */
                const uint32_t c = A.cigar[k++];
                const int op = (int)(c & 0xf);
                const int64_t len = c >> 4;
                if (op == 2) {
                    x += len;
                } else if (op == 0 || op == 7 || op == 8 || op == 1 || op == 4) {
                    match = op != 1 && op != 4;
                    left = len;
                }
            }
            if (left > 0) {
                if (match) {
                    if (x >= A.tab_begin && x < A.tab_end) {
                        v = A.tab[x - A.tab_begin];
                    }
                    x++;
                }
                left--;
            }
        }
        out[i >> 2] |= v << (8 * (i & 3));
    }
    *(uint4 *)(A.bi_out + b0) = make_uint4(out[0], out[1], out[2], out[3]);       /* (BD is the same array: see the head of the file) */
}

int lfq_launch_idq_table(const uint8_t *ref, int64_t ref_len, int64_t tab_begin, int64_t tab_end, uint8_t *tab, void *stream)
{
    if (tab_end <= tab_begin) {
        return LFQ_OK;
    }
    if ((tab_begin & 15) != 0 || tab_end > ref_len) {
        return LFQ_ERR_INVALID;
    }
    const int64_t blocks = (tab_end - tab_begin + LFQ_IDQ_TILE - 1) / LFQ_IDQ_TILE;
    hipLaunchKernelGGL(lfq_idq_table_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ref, ref_len, tab_begin,
                       tab_end, tab);
    return hipGetLastError() == hipSuccess ? LFQ_OK : LFQ_ERR_HIP;
}

int lfq_launch_idq_fill(const LfqIdqArgs &a, void *stream)
{
    if (a.n_bases <= 0) {
        return LFQ_OK;
    }
    const int64_t blocks = ((a.n_bases + 15) / 16 + 255) / 256;
    hipLaunchKernelGGL(lfq_idq_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? LFQ_OK : LFQ_ERR_HIP;
}
