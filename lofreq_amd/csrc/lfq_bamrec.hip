/*
 * lfq_bamrec.hip -- BAM records decoded on the device (lfq_readset_create_from_bam): the bytes of the records go
 * down as they lie in bam1_t.data, an aux pass finds BI / BD per read, a base pass writes the per-base arrays of the read set.
 * The host side that builds the read set around these two launches is in lfq_readset.hip.  For lfq_readset_create_from_bam_tags the
 * aux pass also notes the first lb / ai / ad field, a stored-tag pass lays those strings out per base, and lfq_readset_baq_fill's merge
 * pass puts them over what the HMM kernels computed.  Further down, the way back
 * (lfq_readset_encode_bam): the records rewritten with a read set's results, a plan pass per read and a copy pass per 16 output bytes.
 * Last, lfq_bam_frame_encoded: block_size and the 32 core bytes put in front of every record of the live encode result -- the body
 * of a BAM file, left on the device for lfq_bgzf_deflate.
 *
 * core.bin there is the SAM specification's reg2bin (section 5.3) of the record's new pos and CIGAR.  The reference never sets
 * core.bin after replace_cigar (lofreq_viterbi.c:340), so a realigned record of the 2.1.4 binary can carry the bin of its old
 * alignment: the bin written here is the specification's and not the binary's.
 */
#include "lfq_ctx.h"

#define LFQ_BAM_AUX_READS 256           /* reads per workgroup of the aux pass: one lane each */
#define LFQ_BAM_BASE_CHUNKS 256         /* 16-byte chunks of the destination arrays per workgroup of the base pass: one lane each */

struct LfqBamArgs {
    const uint8_t *data;                /* the records; 4-byte aligned, 16 bytes of slack behind the last record */
    const int64_t *seq_off;             /* [n + 1] */
    const int64_t *seq_src;             /* [n] offset in `data` of the read's first 4-bit base byte */
    const int64_t *rec_end;             /* [n] offset in `data` one past the read's record */
    int64_t *bi_src, *bd_src;           /* [n] offset of the BI / BD string the read counts as having, or -1 (written by the aux pass) */
    uint8_t *flags;                     /* [n] bit 0: BI, bit 1: BD */
    int32_t *err;                       /* [0]: a read has BI, [1]: a read has BD, [2]: a malformed aux field, [3]: see `stored` */
    int64_t *tile_read;                 /* [workgroups of the base pass] the read that holds the first base of the workgroup's tile
                                           (written by the aux pass) */
    int64_t n_reads, n_bases;
    uint8_t *seq, *qual, *bi, *bd;      /* the read set's per-base arrays (16-byte aligned, 16 bytes of slack); bi / bd may be null */
    /* lfq_readset_create_from_bam_tags: the first lb / ai / ad field of a read, in that order */
    uint32_t read_tags;                 /* LFQ_BAM_READ_*: the tags the aux pass looks for (0: none, and nothing below is touched) */
    int64_t *st_src[3];                 /* [n] offset of the string the read has stored, or -1 (written by the aux pass) */
    uint8_t *stored;                    /* [n] bit 0 / 1 / 2: lb / ai / ad stored; err[3]: a first field that cannot be used */
    uint8_t *st_dst[3];                 /* stored-tag pass: the per-base side arrays, laid out as bi / bd; null = no read has the tag */
};

/* the first NUL of [p, end), or a value >= end: four bytes a load, as the aligned dwords that hold them (BI / BD strings are most
 * of a record, and a lane's byte loads are as many memory transactions as a wavefront's dword loads) */
__device__ __forceinline__ int64_t bam_find_nul(const uint8_t *d, int64_t p, int64_t end)
{
    if (p >= end) {
        return end;
    }
    const uint32_t *w = (const uint32_t *)d;
    int64_t a = p >> 2;
    uint32_t x = w[a] | ((1u << ((int)(p & 3) * 8)) - 1u);     /* the bytes in front of p count as non-zero */
    for (;;) {
        const uint32_t z = (x - 0x01010101u) & ~x & 0x80808080u;            /* lowest set bit: the first zero byte */
        if (z) {
            return a * 4 + ((__ffs((int)z) - 1) >> 3);
        }
        a++;
        if (a * 4 >= end) {
            return end;
        }
        x = w[a];
    }
}

/* ---- the aux walk: one field a step ---------------------------------------------------------------------------------------------
 * What both per-read passes (the decode's aux pass, the encode's plan pass) know of an aux field.  This is the only code that reads
 * an aux header or decides a field's size, and so the one place that keeps a lane inside its record: a field whose header, NUL or
 * payload would lie beyond `end` is malformed, decided from the offsets before anything past them is read. */
struct LfqBamAuxField {
    uint8_t t0, t1, ty;                 /* the tag's two bytes, the type */
    int64_t at, size;                   /* the payload: its first byte and its bytes (a string's NUL included) */
    int64_t zlen;                       /* Z / H: the string's length; every other type: -1 */
};

/* the field at *p (< end); false: malformed.  Otherwise *p is behind the field */
__device__ __forceinline__ bool bam_aux_next(const uint8_t *d, int64_t *p_io, int64_t end, LfqBamAuxField *F)
{
    int64_t p = *p_io;
    if (end - p < 3) {
        return false;
    }
    F->t0 = d[p];
    F->t1 = d[p + 1];
    const uint8_t ty = F->ty = d[p + 2];
    p += 3;
    int64_t size = -1, zlen = -1;
    switch (ty) {
    case 'A': case 'c': case 'C':
        size = 1;
        break;
    case 's': case 'S':
        size = 2;
        break;
    case 'i': case 'I': case 'f':
        size = 4;
        break;
    case 'Z': case 'H': {
        const int64_t q = bam_find_nul(d, p, end);
        if (q < end) {
            zlen = q - p;
            size = zlen + 1;
        }
        break;
    }
    case 'B':
        if (end - p >= 5) {
            const uint8_t sub = d[p];
            const int64_t cnt = (int64_t)d[p + 1] | ((int64_t)d[p + 2] << 8) | ((int64_t)d[p + 3] << 16) | ((int64_t)d[p + 4] << 24);
            const int64_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2
                               : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (es) {
                size = 5 + es * cnt;
            }
        }
        break;
    default:
        break;
    }
    if (size < 0 || size > end - p) {
        return false;
    }
    F->at = p;
    F->size = size;
    F->zlen = zlen;
    *p_io = p + size;
    return true;
}

/* ---- aux pass: one lane per read walks the aux fields of its record (bam_aux_next); a malformed field ends the walk and marks
 * the batch malformed */
__global__ __launch_bounds__(LFQ_BAM_AUX_READS) void lfq_bam_aux_kernel(LfqBamArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * LFQ_BAM_AUX_READS + threadIdx.x;
    bool bad = false, has_bi = false, has_bd = false, unusable = false;
    if (r < A.n_reads) {
        const uint8_t *d = A.data;
        const int64_t l = A.seq_off[r + 1] - A.seq_off[r];
        const int64_t end = A.rec_end[r];
        int64_t p = A.seq_src[r] + (l + 1) / 2 + l;
        int64_t bi = -1, bd = -1;
        bool seen_bi = false, seen_bd = false;
        int64_t st[3] = {-1, -1, -1};
        uint32_t seen_st = 0;
        while (p < end) {
            LfqBamAuxField F;
            if (!bam_aux_next(d, &p, end, &F)) {
                bad = true;
                break;
            }
            if (F.t0 == 'B' && F.t1 == 'I' && !seen_bi) {   /* the FIRST field of the tag decides (bam_aux_get) */
                seen_bi = true;
                if (F.ty == 'Z' && F.zlen >= l) {
                    bi = F.at;
                }
            } else if (F.t0 == 'B' && F.t1 == 'D' && !seen_bd) {
                seen_bd = true;
                if (F.ty == 'Z' && F.zlen >= l) {
                    bd = F.at;
                }
            } else if (A.read_tags) {                       /* lb / ai / ad: the first field again, but one that must be usable */
                const int t = (F.t0 == 'l' && F.t1 == 'b') ? 0 : (F.t0 == 'a' && F.t1 == 'i') ? 1 : (F.t0 == 'a' && F.t1 == 'd') ? 2 : -1;
                const uint32_t wanted = (A.read_tags & LFQ_BAM_READ_LB ? 1u : 0u) | (A.read_tags & LFQ_BAM_READ_IDAQ ? 6u : 0u);
                if (t >= 0 && ((wanted >> t) & 1u) && !((seen_st >> t) & 1u)) {
                    seen_st |= 1u << t;
                    if (F.ty == 'Z' && F.zlen >= l) {
                        st[t] = F.at;
                    } else {
                        unusable = true;
                    }
                }
            }
        }
        if (bad) {
            bi = bd = -1;
            st[0] = st[1] = st[2] = -1;
        }
        if (A.read_tags) {
            A.st_src[0][r] = st[0];
            A.st_src[1][r] = st[1];
            A.st_src[2][r] = st[2];
            A.stored[r] = (uint8_t)((st[0] >= 0 ? 1 : 0) | (st[1] >= 0 ? 2 : 0) | (st[2] >= 0 ? 4 : 0));
        }
        has_bi = bi >= 0;
        has_bd = bd >= 0;
        /* the base pass finds the reads of a tile here instead of searching seq_off */
        const int64_t tile = (int64_t)LFQ_BAM_BASE_CHUNKS * 16, so = A.seq_off[r];
        for (int64_t t = (so + tile - 1) / tile; t * tile < so + l; t++) {
            A.tile_read[t] = r;
        }
        A.bi_src[r] = bi;
        A.bd_src[r] = bd;
        A.flags[r] = (uint8_t)((has_bi ? 1 : 0) | (has_bd ? 2 : 0));
    }
    const bool any_bi = __any(has_bi), any_bd = __any(has_bd), any_bad = __any(bad), any_unusable = __any(unusable);
    if ((threadIdx.x & 63) == 0) {
        if (any_bi) atomicOr(&A.err[0], 1);
        if (any_bd) atomicOr(&A.err[1], 1);
        if (any_bad) atomicOr(&A.err[2], 1);
        if (any_unusable) atomicOr(&A.err[3], 1);
    }
}

/* ---- base pass: output-major, one lane per 16 bytes of the destination arrays -----------------------------------------------
 * 16 bytes in two registers pairs; byte k of the chunk is byte k of the value */
struct LfqB16 {
    uint64_t lo, hi;
};

__device__ __forceinline__ LfqB16 b16_shl_bytes(LfqB16 v, int nbytes)       /* 0 .. 15 */
{
    const int s = nbytes * 8;
    LfqB16 o;
    if (s == 0) {
        o = v;
    } else if (s >= 64) {
        o.lo = 0;
        o.hi = v.lo << (s - 64);
    } else {
        o.lo = v.lo << s;
        o.hi = (v.hi << s) | (v.lo >> (64 - s));
    }
    return o;
}

__device__ __forceinline__ LfqB16 b16_mask(int cnt)                         /* the first cnt (1 .. 16) bytes */
{
    LfqB16 m;
    m.lo = cnt >= 8 ? ~0ull : ((1ull << (cnt * 8)) - 1);
    m.hi = cnt >= 16 ? ~0ull : cnt > 8 ? ((1ull << ((cnt - 8) * 8)) - 1) : 0ull;
    return m;
}

/* cnt (1 .. 16) bytes from byte offset s of the records, read as the aligned dwords that hold them -- at most 3 bytes before
 * the first and 3 behind the last one, which the buffer's alignment and slack cover; the bytes behind cnt are 0 */
__device__ __forceinline__ LfqB16 b16_fetch(const uint8_t *data, int64_t s, int cnt)
{
    const uint32_t *w32 = (const uint32_t *)data + (s >> 2);
    const int sh = (int)(s & 3) * 8;
    const int nd = ((int)(s & 3) + cnt + 3) >> 2;                           /* 1 .. 5 */
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        w[i] = i < nd ? w32[i] : 0u;
    }
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        o[i] = (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> sh);
    }
    const LfqB16 m = b16_mask(cnt);
    LfqB16 v;
    v.lo = (o[0] | ((uint64_t)o[1] << 32)) & m.lo;
    v.hi = (o[2] | ((uint64_t)o[3] << 32)) & m.hi;
    return v;
}

/* cnt (1 .. 16) base codes of a read from its base i0 on.  The 4-bit BAM base "=ACMGRSVTWYHKDBN" -> the library's code: 0..3 =
 * A, C, G, T, 4 = N, 5..15 = the other letters in the order "=MRSVWYHKDB" (include/lofreq_amd.h); the table is a register pair */
__device__ __forceinline__ LfqB16 b16_bases(const uint8_t *data, int64_t seq_src, int64_t i0, int cnt)
{
    const uint64_t T0 = 0x0908070206010005ull, T1 = 0x040f0e0d0c0b0a03ull;
    const int odd = (int)(i0 & 1);
    LfqB16 v = b16_fetch(data, seq_src + (i0 >> 1), (odd + cnt + 1) >> 1);  /* at most 9 bytes */
    /* high nibble first -> nibble k at bit 4 k, then the first base to bit 0 */
    v.lo = ((v.lo & 0x0f0f0f0f0f0f0f0full) << 4) | ((v.lo >> 4) & 0x0f0f0f0f0f0f0f0full);
    v.hi = ((v.hi & 0x0f0f0f0f0f0f0f0full) << 4) | ((v.hi >> 4) & 0x0f0f0f0f0f0f0f0full);
    const uint64_t nib = odd ? (v.lo >> 4) | (v.hi << 60) : v.lo;
    LfqB16 o;
    o.lo = o.hi = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t a = (uint32_t)(nib >> (4 * j)) & 0xf, b = (uint32_t)(nib >> (4 * (j + 8))) & 0xf;
        o.lo |= (((a & 8) ? T1 : T0) >> ((a & 7) * 8) & 0xff) << (8 * j);
        o.hi |= (((b & 8) ? T1 : T0) >> ((b & 7) * 8) & 0xff) << (8 * j);
    }
    const LfqB16 m = b16_mask(cnt);
    o.lo &= m.lo;
    o.hi &= m.hi;
    return o;
}

__device__ __forceinline__ void b16_store(uint8_t *dst, LfqB16 v)
{
    *(uint4 *)dst = make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
}

/* the first read r of [lo, hi] with seq_off[r + 1] > b: the read that holds base b (reads without bases are stepped over) */
__device__ __forceinline__ int64_t bam_read_of_base(const int64_t *seq_off, int64_t lo, int64_t hi, int64_t b)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seq_off[mid + 1] > b) {
            hi = mid;
        } else {
            lo = mid + 1;
        }
    }
    return lo;
}

__global__ __launch_bounds__(LFQ_BAM_BASE_CHUNKS) void lfq_bam_bases_kernel(LfqBamArgs A)
{
    /* the reads of the workgroup's 4096 bases: from the first read of this tile to the first read of the next one (the aux pass
     * wrote both down); a lane looks for its chunk's first read among those few -- 27 reads of 150 bases -- and walks on */
    const int64_t tile0 = (int64_t)blockIdx.x * LFQ_BAM_BASE_CHUNKS * 16;
    const int64_t b0 = tile0 + (int64_t)threadIdx.x * 16;
    if (b0 >= A.n_bases) {
        return;
    }
    const int64_t r_lo = A.tile_read[blockIdx.x], r_hi = blockIdx.x + 1 < gridDim.x ? A.tile_read[blockIdx.x + 1] : A.n_reads - 1;
    const int total = (int)min((int64_t)16, A.n_bases - b0);
    int64_t r = bam_read_of_base(A.seq_off, r_lo, r_hi, b0);
    LfqB16 vs, vq, vi, vd;
    vs.lo = vs.hi = vq.lo = vq.hi = vi.lo = vi.hi = vd.lo = vd.hi = 0;
    int j = 0;
    while (j < total) {                 /* one round per read the chunk touches: one for 9 chunks in 10 of 150-base reads */
        const int64_t b = b0 + j;
        while (A.seq_off[r + 1] <= b) {
            r++;
        }
        const int64_t so = A.seq_off[r], e = A.seq_off[r + 1], i0 = b - so, l = e - so;
        const int cnt = (int)min(e - b, (int64_t)(total - j));
        const int64_t src = A.seq_src[r];
        const LfqB16 ps = b16_shl_bytes(b16_bases(A.data, src, i0, cnt), j);
        const LfqB16 pq = b16_shl_bytes(b16_fetch(A.data, src + (l + 1) / 2 + i0, cnt), j);
        vs.lo |= ps.lo; vs.hi |= ps.hi;
        vq.lo |= pq.lo; vq.hi |= pq.hi;
        if (A.bi || A.bd) {
            LfqB16 none = b16_mask(cnt);                    /* a read without the tag: '!' */
            none.lo &= 0x2121212121212121ull;
            none.hi &= 0x2121212121212121ull;
            if (A.bi) {
                const int64_t s = A.bi_src[r];
                const LfqB16 pi = b16_shl_bytes(s >= 0 ? b16_fetch(A.data, s + i0, cnt) : none, j);
                vi.lo |= pi.lo; vi.hi |= pi.hi;
            }
            if (A.bd) {
                const int64_t s = A.bd_src[r];
                const LfqB16 pd = b16_shl_bytes(s >= 0 ? b16_fetch(A.data, s + i0, cnt) : none, j);
                vd.lo |= pd.lo; vd.hi |= pd.hi;
            }
        }
        j += cnt;
    }
    b16_store(A.seq + b0, vs);
    b16_store(A.qual + b0, vq);
    if (A.bi) b16_store(A.bi + b0, vi);
    if (A.bd) b16_store(A.bd + b0, vd);
}

/* ---- stored-tag pass: the base pass's sibling for the first lb / ai / ad strings, same tiles, same chunks; a read without the tag
 * holds '!' throughout */
__global__ __launch_bounds__(LFQ_BAM_BASE_CHUNKS) void lfq_bam_stored_kernel(LfqBamArgs A)
{
    const int64_t tile0 = (int64_t)blockIdx.x * LFQ_BAM_BASE_CHUNKS * 16;
    const int64_t b0 = tile0 + (int64_t)threadIdx.x * 16;
    if (b0 >= A.n_bases) {
        return;
    }
    const int64_t r_lo = A.tile_read[blockIdx.x], r_hi = blockIdx.x + 1 < gridDim.x ? A.tile_read[blockIdx.x + 1] : A.n_reads - 1;
    const int total = (int)min((int64_t)16, A.n_bases - b0);
    int64_t r = bam_read_of_base(A.seq_off, r_lo, r_hi, b0);
    LfqB16 v[3];
    v[0].lo = v[0].hi = v[1].lo = v[1].hi = v[2].lo = v[2].hi = 0;
    int j = 0;
    while (j < total) {
        const int64_t b = b0 + j;
        while (A.seq_off[r + 1] <= b) {
            r++;
        }
        const int64_t so = A.seq_off[r], e = A.seq_off[r + 1], i0 = b - so;
        const int cnt = (int)min(e - b, (int64_t)(total - j));
        LfqB16 none = b16_mask(cnt);
        none.lo &= 0x2121212121212121ull;
        none.hi &= 0x2121212121212121ull;
#pragma unroll
        for (int t = 0; t < 3; t++) {
            if (A.st_dst[t]) {
                const int64_t s = A.st_src[t][r];
                const LfqB16 pt = b16_shl_bytes(s >= 0 ? b16_fetch(A.data, s + i0, cnt) : none, j);
                v[t].lo |= pt.lo; v[t].hi |= pt.hi;
            }
        }
        j += cnt;
    }
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (A.st_dst[t]) b16_store(A.st_dst[t] + b0, v[t]);
    }
}

/* ---- merge pass (lfq_readset_baq_fill): per read and tag the stored bytes replace the computed ones.  One lane owns one 16-byte
 * chunk of the destination arrays and rewrites it under a byte mask built from the reads it spans -- neighbouring reads of a chunk
 * differ in what they have stored -- so there are no byte stores and no two lanes write one chunk.  take[r] bit t: read r takes
 * its stored tag t (lb, ai, ad). */
struct LfqBamMergeArgs {
    const int64_t *seq_off;             /* [n + 1] the read set's */
    const uint8_t *take;                /* [n] */
    const uint8_t *src[3];              /* the stored side arrays; null = the tag is not merged */
    uint8_t *dst[3];                    /* the read set's lb, ai, ad (16-byte aligned, 16 bytes of slack) */
    uint8_t *tagfl;                     /* [n] bit 0 / 1: the read has ai / ad (null: no ai / ad in this fill) */
    int64_t n_reads, n_bases;
};

__global__ __launch_bounds__(LFQ_BAM_BASE_CHUNKS) void lfq_bam_merge_kernel(LfqBamMergeArgs A)
{
    const int64_t b0 = ((int64_t)blockIdx.x * LFQ_BAM_BASE_CHUNKS + threadIdx.x) * 16;
    if (b0 >= A.n_bases) {
        return;
    }
    const int total = (int)min((int64_t)16, A.n_bases - b0);
    int64_t r = bam_read_of_base(A.seq_off, 0, A.n_reads - 1, b0);
    LfqB16 m[3];
    m[0].lo = m[0].hi = m[1].lo = m[1].hi = m[2].lo = m[2].hi = 0;
    int j = 0;
    while (j < total) {
        const int64_t b = b0 + j;
        while (A.seq_off[r + 1] <= b) {
            r++;
        }
        const int cnt = (int)min(A.seq_off[r + 1] - b, (int64_t)(total - j));
        const uint32_t tk = A.take[r];
        const LfqB16 mr = b16_shl_bytes(b16_mask(cnt), j);
#pragma unroll
        for (int t = 0; t < 3; t++) {
            if ((tk >> t) & 1u) {
                m[t].lo |= mr.lo; m[t].hi |= mr.hi;
            }
        }
        j += cnt;
    }
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (A.src[t] && (m[t].lo | m[t].hi)) {
            const uint4 s = *(const uint4 *)(A.src[t] + b0), d = *(const uint4 *)(A.dst[t] + b0);
            LfqB16 o;
            o.lo = ((((uint64_t)d.y << 32) | d.x) & ~m[t].lo) | ((((uint64_t)s.y << 32) | s.x) & m[t].lo);
            o.hi = ((((uint64_t)d.w << 32) | d.z) & ~m[t].hi) | ((((uint64_t)s.w << 32) | s.z) & m[t].hi);
            b16_store(A.dst[t] + b0, o);
        }
    }
}

/* the stored ai / ad bits join what the BAQ kernels wrote, in front of lfq_launch_flag_merge */
__global__ __launch_bounds__(256) void lfq_bam_merge_flags_kernel(uint8_t *tagfl, const uint8_t *take, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        tagfl[i] = (uint8_t)(tagfl[i] | ((take[i] >> 1) & 3u));
    }
}

/* ---- host side: what the decode and the encode keep on a context, and the upload both begin with --------------------------- */
struct LfqBamState {
    uint8_t *d_buf = nullptr;           /* records | descriptors | what the aux or the plan pass writes (grow-only) */
    int64_t d_bytes = 0;
    uint8_t *h_stage = nullptr;         /* pinned staging of records that come in pageable memory (grow-only) */
    int64_t h_bytes = 0;
    LfqEvPair up_t = {}, kern_t = {}, down_t = {};      /* around a call's copies down, a kernel, the copies back; each is read
                                                           (after the call's next synchronise) before it is recorded again */
    /* lfq_readset_create_from_bam */
    LfqBamArgs args = {};               /* of the decode in flight between lfq_bam_aux and lfq_bam_bases */
    lfq_bam_decode_times times = {};
    /* lfq_readset_encode_bam */
    uint8_t *d_out = nullptr;           /* offsets | tile table | the blob (grow-only) */
    int64_t d_out_bytes = 0;
    uint8_t *h_out = nullptr;           /* the blob on the host, pinned (grow-only) */
    int64_t h_out_bytes = 0;
    std::vector<int64_t> data_off, src;
    std::vector<int32_t> pos;
    std::vector<uint32_t> n_cigar;
    uint8_t none[16] = {};              /* `data` of an empty result */
    lfq_bam_encoded result = {};
    lfq_bam_encode_times enc_times = {};
    /* lfq_bam_frame_encoded: what it needs of the encode result, which stays in d_out (offsets at its front) */
    bool enc_live = false;              /* `result` and d_out hold a complete encode */
    int64_t enc_blob = 0;               /* where the blob starts in d_out */
    std::vector<uint16_t> enc_lq;       /* [n] l_qname / l_qseq of the record read j was made from */
    std::vector<int32_t> enc_ls;
    uint8_t *d_frame = nullptr;         /* cores | src | pos | n_cigar | new cores | the body (grow-only) */
    int64_t d_frame_bytes = 0;
    uint8_t *h_frame = nullptr;         /* the body on the host, pinned (grow-only) */
    int64_t h_frame_bytes = 0;
    int64_t frame_live = 0, frame_body = 0;     /* bytes of the live body at framed.data (0: none); where it starts in d_frame */
    std::vector<int64_t> rec_off;
    lfq_bam_framed framed = {};
};

static LfqBamState *bam_state(lfq_ctx *c)
{
    if (!c->bam) {
        c->bam = new LfqBamState();
    }
    return c->bam;
}

void lfq_bam_release(lfq_ctx *c)
{
    if (LfqBamState *S = c->bam) {
        if (S->d_buf) (void)hipFree(S->d_buf);
        if (S->d_out) (void)hipFree(S->d_out);
        free_pinned(&S->h_stage, &S->h_bytes);
        free_pinned(&S->h_out, &S->h_out_bytes);
        if (S->d_frame) (void)hipFree(S->d_frame);
        free_pinned(&S->h_frame, &S->h_frame_bytes);
        for (LfqEvPair *t : {&S->up_t, &S->kern_t, &S->down_t}) {
            t->destroy();
        }
        delete S;
        c->bam = nullptr;
    }
}

void lfq_bam_times_reset(lfq_ctx *c, int64_t n_reads, int64_t n_bases, int64_t n_data_bytes)
{
    LfqBamState *S = bam_state(c);
    S->times = {};
    S->times.n_reads = n_reads;
    S->times.n_bases = n_bases;
    S->times.n_data_bytes = n_data_bytes;
}

/* the pair's milliseconds on top of *acc: a leg of the encode has two parts, the kernels of both calls are two launches */
static int bam_add_ms(const LfqEvPair &t, double *acc)
{
    double ms = 0.0;
    LFQ_TRY(t.ms(&ms));
    *acc += ms;
    return LFQ_OK;
}

/* records that come in pageable memory: *data becomes their copy in the pinned staging area */
static int bam_stage(LfqBamState *S, const uint8_t **data_io, int64_t data_bytes)
{
    const uint8_t *data = *data_io;
    if (data_bytes > S->h_bytes) {      /* a quarter over the need: batches of about one size do not allocate again */
        LFQ_TRY(grow_pinned(&S->h_stage, &S->h_bytes, std::max<int64_t>(data_bytes + data_bytes / 4, 1 << 16)));
    }
    /* (a few threads: one copies at a fraction of what the link takes) */
    const unsigned hw = std::max(1u, lfq_cpu_budget() / (unsigned)std::max(lfq_knobs().local_world_size, 1));
    const int parts = data_bytes >= ((int64_t)32 << 20) ? (int)std::min(8u, hw) : 1;
    uint8_t *stage = S->h_stage;
    auto copy_part = [=](int p) {
        const int64_t a = data_bytes * p / parts, b = data_bytes * (p + 1) / parts;
        memcpy(stage + a, data + a, (size_t)(b - a));
    };
    std::vector<std::thread> th;
    for (int p = 1; p < parts; p++) {
        th.emplace_back(copy_part, p);
    }
    copy_part(0);
    for (auto &t : th) {
        t.join();
    }
    *data_io = S->h_stage;
    return LFQ_OK;
}

/* the leg both calls begin with, inside up_t: d_buf grown to `total`; the records down, behind first_shift bytes of room so that a
 * record keeps the alignment it has in the caller's buffer, through the staging area unless they lie in pinned memory -- or device
 * to device when they lie in the context's live lfq_bgzf_inflate result, whose bytes are still resident (lfq_bgzf.hip); the call's
 * per-read descriptors down to o_desc; the 256 bytes of the error words at o_err cleared */
static int bam_upload(lfq_ctx *c, LfqBamState *S, const LfqBamIn &in, int64_t total, int64_t o_desc, const void *desc,
                      size_t desc_bytes, int64_t o_err)
{
    LFQ_TRY(grow(&S->d_buf, &S->d_bytes, total));
    const uint8_t *data = in.data;
    /* records inside the context's live lfq_bgzf_inflate result are on the device already: they do not cross the link again */
    const uint8_t *resident = in.data_bytes > 0 ? lfq_bgzf_resident(c, in.data, in.data_bytes) : nullptr;
    if (!resident && !in.pinned) {
        LFQ_TRY(bam_stage(S, &data, in.data_bytes));
    }
    hipStream_t st = c->stream;
    LFQ_TRY(S->up_t.begin(st));
    if (resident) {
        LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf + in.first_shift, resident, (size_t)in.data_bytes, hipMemcpyDeviceToDevice, st));
    } else {
        LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf + in.first_shift, data, (size_t)in.data_bytes, hipMemcpyHostToDevice, st));
    }
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf + o_desc, desc, desc_bytes, hipMemcpyHostToDevice, st));
    LFQ_TRY_HIP(hipMemsetAsync(S->d_buf + o_err, 0, 256, st));
    return S->up_t.end(st);
}

/* ---- host side of the decode's two launches ---------------------------------------------------------------------------------- */
/* records down, aux pass, its verdict back: flags_out[n], *any_bi / *any_bd; LFQ_ERR_INVALID for a malformed aux field.
 * desc = seq_off[n + 1] | seq_src[n] | rec_end[n], the last two as offsets from in.data - in.first_shift.  Blocks. */
int lfq_bam_aux(lfq_ctx *c, const LfqBamIn &in, const int64_t *desc, int64_t n, int64_t nb, uint8_t *flags_out, int *any_bi,
                int *any_bd, unsigned read_tags, uint8_t *stored_out)
{
    LfqBamState *S = bam_state(c);
    LFQ_TRY_HIP(hipSetDevice(c->device));
    /* (read_tags: three more offset arrays and the stored bits behind the tile table) */
    const int64_t o_desc = lfq_al(in.first_shift + in.data_bytes + 16), o_bi = o_desc + lfq_al((3 * n + 1) * 8),
                  o_bd = o_bi + lfq_al(n * 8), o_err = o_bd + lfq_al(n * 8), o_fl = o_err + 256, o_tile = o_fl + lfq_al(n),
                  n_tiles = (nb + LFQ_BAM_BASE_CHUNKS * 16 - 1) / (LFQ_BAM_BASE_CHUNKS * 16), o_st = o_tile + lfq_al(n_tiles * 8),
                  o_sfl = o_st + (read_tags ? 3 * lfq_al(n * 8) : 0), total = o_sfl + (read_tags ? lfq_al(n) : 0);
    LfqPin<int32_t> verdict(c, 4);
    LFQ_PIN_OK(verdict);
    LfqPin<uint8_t> fl(c, (size_t)n);
    LFQ_PIN_OK(fl);
    LfqPin<uint8_t> sfl(c, (size_t)n);
    LFQ_PIN_OK(sfl);
    LFQ_TRY(bam_upload(c, S, in, total, o_desc, desc, (size_t)(3 * n + 1) * 8, o_err));
    hipStream_t st = c->stream;
    LfqBamArgs &A = S->args;
    memset(&A, 0, sizeof(A));
    A.data = S->d_buf;
    A.seq_off = (const int64_t *)(S->d_buf + o_desc);
    A.seq_src = A.seq_off + n + 1;
    A.rec_end = A.seq_src + n;
    A.bi_src = (int64_t *)(S->d_buf + o_bi);
    A.bd_src = (int64_t *)(S->d_buf + o_bd);
    A.err = (int32_t *)(S->d_buf + o_err);
    A.flags = S->d_buf + o_fl;
    A.tile_read = (int64_t *)(S->d_buf + o_tile);
    A.n_reads = n;
    A.n_bases = nb;
    A.read_tags = read_tags;
    if (read_tags) {
        for (int t = 0; t < 3; t++) {
            A.st_src[t] = (int64_t *)(S->d_buf + o_st + t * lfq_al(n * 8));
        }
        A.stored = S->d_buf + o_sfl;
    }
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bam_aux_kernel, dim3((unsigned)((n + LFQ_BAM_AUX_READS - 1) / LFQ_BAM_AUX_READS)),
                       dim3(LFQ_BAM_AUX_READS), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    S->times.n_launches += 1;
    LFQ_TRY_HIP(hipMemcpyAsync(verdict.data(), A.err, 16, hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipMemcpyAsync(fl.data(), A.flags, (size_t)n, hipMemcpyDeviceToHost, st));
    if (read_tags) {
        LFQ_TRY_HIP(hipMemcpyAsync(sfl.data(), A.stored, (size_t)n, hipMemcpyDeviceToHost, st));
    }
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bam_add_ms(S->up_t, &S->times.upload_ms));
    LFQ_TRY(bam_add_ms(S->kern_t, &S->times.kernels_ms));
    if (verdict[2] || verdict[3]) {     /* malformed, or a first lb / ai / ad field that is no string of l_qseq bytes */
        return LFQ_ERR_INVALID;
    }
    memcpy(flags_out, fl.data(), (size_t)n);
    if (read_tags) {
        memcpy(stored_out, sfl.data(), (size_t)n);
    }
    *any_bi = verdict[0] != 0;
    *any_bd = verdict[1] != 0;
    return LFQ_OK;
}

/* base pass of the decode lfq_bam_aux began, into the read set's device arrays (d_bi / d_bd null: the read set has none), and
 * their copies back into the pinned host arrays.  Blocks. */
int lfq_bam_bases(lfq_ctx *c, uint8_t *d_seq, uint8_t *d_qual, uint8_t *d_bi, uint8_t *d_bd, uint8_t *h_seq, uint8_t *h_qual,
                  uint8_t *h_bi, uint8_t *h_bd)
{
    LfqBamState *S = bam_state(c);
    LfqBamArgs A = S->args;
    const int64_t nb = A.n_bases;
    if (nb <= 0) {
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    A.seq = d_seq; A.qual = d_qual; A.bi = d_bi; A.bd = d_bd;
    const int64_t per_wg = (int64_t)LFQ_BAM_BASE_CHUNKS * 16;
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bam_bases_kernel, dim3((unsigned)((nb + per_wg - 1) / per_wg)), dim3(LFQ_BAM_BASE_CHUNKS), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    S->times.n_launches += 1;
    LFQ_TRY(S->down_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(h_seq, d_seq, (size_t)nb, hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipMemcpyAsync(h_qual, d_qual, (size_t)nb, hipMemcpyDeviceToHost, st));
    if (d_bi) {
        LFQ_TRY_HIP(hipMemcpyAsync(h_bi, d_bi, (size_t)nb, hipMemcpyDeviceToHost, st));
    }
    if (d_bd) {
        LFQ_TRY_HIP(hipMemcpyAsync(h_bd, d_bd, (size_t)nb, hipMemcpyDeviceToHost, st));
    }
    LFQ_TRY(S->down_t.end(st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bam_add_ms(S->kern_t, &S->times.kernels_ms));
    return bam_add_ms(S->down_t, &S->times.download_ms);
}

/* stored-tag pass of the decode lfq_bam_aux began.  Blocks (the records below it are the context's until the next decode). */
int lfq_bam_stored(lfq_ctx *c, uint8_t *const d_dst[3])
{
    LfqBamState *S = bam_state(c);
    LfqBamArgs A = S->args;
    const int64_t nb = A.n_bases;
    if (nb <= 0 || !A.read_tags || (!d_dst[0] && !d_dst[1] && !d_dst[2])) {
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    for (int t = 0; t < 3; t++) {
        A.st_dst[t] = d_dst[t];
    }
    const int64_t per_wg = (int64_t)LFQ_BAM_BASE_CHUNKS * 16;
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bam_stored_kernel, dim3((unsigned)((nb + per_wg - 1) / per_wg)), dim3(LFQ_BAM_BASE_CHUNKS), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    S->times.n_launches += 1;
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    return bam_add_ms(S->kern_t, &S->times.kernels_ms);
}

/* merge pass of lfq_readset_baq_fill, queued on `st` */
int lfq_bam_merge(const int64_t *d_seq_off, const uint8_t *d_take, const uint8_t *const d_src[3], uint8_t *const d_dst[3],
                  uint8_t *d_tagfl, int64_t n, int64_t nb, hipStream_t st)
{
    if (n <= 0) {
        return LFQ_OK;
    }
    LfqBamMergeArgs M;
    memset(&M, 0, sizeof(M));
    M.seq_off = d_seq_off;
    M.take = d_take;
    bool any = false;
    for (int t = 0; t < 3; t++) {
        M.src[t] = d_dst[t] ? d_src[t] : nullptr;
        M.dst[t] = d_dst[t];
        any = any || M.src[t];
    }
    M.tagfl = d_tagfl;
    M.n_reads = n;
    M.n_bases = nb;
    const int64_t per_wg = (int64_t)LFQ_BAM_BASE_CHUNKS * 16;
    if (any && nb > 0) {
        hipLaunchKernelGGL(lfq_bam_merge_kernel, dim3((unsigned)((nb + per_wg - 1) / per_wg)), dim3(LFQ_BAM_BASE_CHUNKS), 0, st, M);
        LFQ_TRY_HIP(hipGetLastError());
    }
    if (d_tagfl) {
        hipLaunchKernelGGL(lfq_bam_merge_flags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_tagfl, d_take, n);
        LFQ_TRY_HIP(hipGetLastError());
    }
    return LFQ_OK;
}

extern "C" int lfq_last_bam_decode_times(lfq_ctx *c, lfq_bam_decode_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = bam_state(c)->times;
    return LFQ_OK;
}

/* ==== the way back: lfq_readset_encode_bam =======================================================================================
 * The records of a read set rewritten on the device (include/lofreq_amd.h has the rules): a plan pass, one lane per read, walks
 * the aux fields of the read's record once and writes down which byte ranges survive, which of lb / ai / ad / BI / BD are appended
 * and how long the new record is; the host makes offsets of the lengths; a copy pass, output-major like the base pass of the
 * decode, writes the blob. */
#define LFQ_BAM_PLAN_READS 256          /* reads per workgroup of the plan pass: one lane each */
#define LFQ_BAM_COPY_CHUNKS 256         /* 16-byte chunks of the output blob per workgroup of the copy pass: one lane each */
#define LFQ_BAM_MAX_KEEP 10             /* NM MC MD AS lb ai ad BI BD: at most 9 removed fields, 10 surviving ranges around them */
#define LFQ_BAM_N_APPEND 5              /* lb ai ad BI BD, in the order they are appended */
#define LFQ_BAM_N_SEGMENTS (3 + LFQ_BAM_MAX_KEEP + 3 * LFQ_BAM_N_APPEND)

struct LfqBamPlan {                     /* per read, written by the plan pass */
    int32_t keep_beg[LFQ_BAM_MAX_KEEP]; /* surviving ranges of the aux block, from the record's first byte */
    int32_t keep_len[LFQ_BAM_MAX_KEEP];
    int32_t n_keep;
    uint32_t append;                    /* bit f: field f of lb ai ad BI BD is appended */
};

struct LfqBamEncArgs {
    const uint8_t *data;                /* the records; 4-byte aligned, 16 bytes of slack behind the last record */
    const LfqBamRead *reads;            /* [n] */
    LfqBamPlan *plan;                   /* [n] */
    int64_t *out_len;                   /* [n] bytes of the new record (plan pass) */
    int32_t *err;                       /* [0]: a malformed aux field */
    const int64_t *out_off;             /* [n + 1] (host) */
    const int64_t *tile_rec;            /* [workgroups of the copy pass] the read whose record holds the first byte of the tile (host) */
    const int64_t *coff, *soff;         /* the read set's */
    const uint32_t *cig;
    const uint8_t *fl;
    const uint8_t *lb, *ai, *ad, *bi, *bd;
    uint8_t *out;                       /* 16-byte aligned, 16 bytes of slack */
    int64_t n_reads, n_out;
    uint32_t what;
    int32_t uniform;
};

/* ---- plan pass: one lane per read walks the aux fields of its record (bam_aux_next) under the reference's deletion and append
 * rules */
__global__ __launch_bounds__(LFQ_BAM_PLAN_READS) void lfq_bam_plan_kernel(LfqBamEncArgs A)
{
    const int64_t j = (int64_t)blockIdx.x * LFQ_BAM_PLAN_READS + threadIdx.x;
    bool bad = false;
    if (j < A.n_reads) {
        const LfqBamRead R = A.reads[j];
        const uint8_t *d = A.data;
        const int64_t l = R.l_qseq, end = R.end;
        const int64_t fixed = (int64_t)R.l_qname + 4 * (int64_t)R.n_cigar + (l + 1) / 2 + l, aux0 = R.rec + fixed;
        const int64_t c0 = A.coff[j], c1 = A.coff[j + 1];
        bool has_ins = false, has_del = false;
        for (int64_t k = c0; k < c1; k++) {
            const uint32_t op = A.cig[k] & 0xf;
            has_ins = has_ins || op == 1;
            has_del = has_del || op == 2;
        }
        const bool put_lb = (A.what & LFQ_BAM_PUT_LB) != 0, put_idaq = (A.what & LFQ_BAM_PUT_IDAQ) != 0;
        const bool alnq = (put_lb || put_idaq) && !(R.flag & 4) && l > 0;                     /* bam_md_ext.c:291 */
        const bool idq = (A.what & LFQ_BAM_PUT_INDELQUAL) && (A.uniform || !(R.flag & 0x704));  /* lofreq_indelqual.c:143-148 */
        const bool drop = (A.what & LFQ_BAM_DROP_ALN_TAGS) != 0, keep_existing = (A.what & LFQ_BAM_KEEP_EXISTING) != 0;
        uint32_t seen = 0;              /* bit 0..3: NM MC MD AS, 4..6: lb ai ad, 7..8: BI BD -- the FIRST field of a tag decides */
        uint32_t present = 0;           /* bit 0..2: P_lb, P_ai, P_ad */
        LfqBamPlan *P = A.plan + j;
        int nk = 0;
        int64_t kept = 0, run = aux0, p = aux0;
        while (p < end) {
            const int64_t f0 = p;
            LfqBamAuxField F;
            if (!bam_aux_next(d, &p, end, &F)) {
                bad = true;
                break;
            }
            const int64_t f1 = p;
            int id = -1;
            switch (((uint32_t)F.t0 << 8) | F.t1) {
            case ('N' << 8) | 'M': id = 0; break;
            case ('M' << 8) | 'C': id = 1; break;
            case ('M' << 8) | 'D': id = 2; break;
            case ('A' << 8) | 'S': id = 3; break;
            case ('l' << 8) | 'b': id = 4; break;
            case ('a' << 8) | 'i': id = 5; break;
            case ('a' << 8) | 'd': id = 6; break;
            case ('B' << 8) | 'I': id = 7; break;
            case ('B' << 8) | 'D': id = 8; break;
            default: break;
            }
            bool del = false;
            if (id >= 0 && !((seen >> id) & 1u)) {
                if (id < 4) {
                    if (drop) {                             /* lofreq_viterbi.c:119-146: any type, every record */
                        seen |= 1u << id;
                        del = true;
                    }
                } else if (id < 7) {
                    if (alnq) {                             /* bam_md_ext.c:297-314 */
                        seen |= 1u << id;
                        const bool selected = id == 4 ? put_lb : put_idaq;
                        if (!keep_existing && selected && F.ty == 'Z') {
                            del = true;
                        } else {
                            present |= 1u << (id - 4);
                        }
                    }
                } else if (idq) {                           /* lofreq_indelqual.c:69-104 */
                    seen |= 1u << id;
                    del = true;
                }
            }
            if (del) {
                if (f0 > run && nk < LFQ_BAM_MAX_KEEP) {    /* (adjacent removals merge: nothing lies between them) */
                    P->keep_beg[nk] = (int32_t)(run - R.rec);
                    P->keep_len[nk] = (int32_t)(f0 - run);
                    kept += f0 - run;
                    nk++;
                }
                run = f1;
            }
        }
        uint32_t app = 0;
        if (bad) {
            nk = 0;
            kept = 0;
        } else {
            if (end > run && nk < LFQ_BAM_MAX_KEEP) {
                P->keep_beg[nk] = (int32_t)(run - R.rec);
                P->keep_len[nk] = (int32_t)(end - run);
                kept += end - run;
                nk++;
            }
            if (alnq) {
                const bool p_lb = present & 1u, p_ai = present & 2u, p_ad = present & 4u;
                const bool skip = (!put_lb || p_lb) && (!has_del || p_ad) && (!has_ins || p_ai);      /* bam_md_ext.c:352-366 */
                if (!skip) {
                    if (put_lb && !p_lb) {
                        app |= 1u;
                    }
                    if (put_idaq && (has_ins || has_del)) { /* whatever P_ai / P_ad say (:241-246) */
                        const uint8_t tf = A.fl[j];
                        app |= ((tf & 4u) ? 2u : 0u) | ((tf & 8u) ? 4u : 0u);
                    }
                }
            }
            if (idq) {
                app |= 8u | 16u;
            }
        }
        P->n_keep = nk;
        P->append = app;
        const int64_t nc_out = (A.what & LFQ_BAM_PUT_ALIGNMENT) ? c1 - c0 : (int64_t)R.n_cigar;
        A.out_len[j] = bad ? 0 : fixed - 4 * (int64_t)R.n_cigar + 4 * nc_out + kept + (int64_t)__popc(app) * (l + 4);
    }
    const bool any_bad = __any(bad);
    if ((threadIdx.x & 63) == 0 && any_bad) {
        atomicOr(&A.err[0], 1);
    }
}

/* ---- copy pass: output-major, one lane per 16 bytes of the blob, one aligned 16-byte store per lane --------------------------------
 * A new record is a list of LFQ_BAM_N_SEGMENTS segments, empty ones included: qname, CIGAR words, seq + qual, the surviving aux
 * ranges, and per appended field its 3-byte head, its l_qseq bytes and its NUL.  Segment k of read j: `len` bytes from byte `src`
 * of `base`, or -- base null -- the bytes of `cval`. */
__device__ __forceinline__ void bam_enc_segment(const LfqBamEncArgs &A, int64_t j, const LfqBamRead &R, int k, const uint8_t **base,
                                                int64_t *src, int64_t *len, uint32_t *cval)
{
    const int64_t l = R.l_qseq;
    *base = A.data;
    *cval = 0;
    if (k == 0) {
        *src = R.rec;
        *len = R.l_qname;
    } else if (k == 1) {
        if (A.what & LFQ_BAM_PUT_ALIGNMENT) {
            const int64_t c0 = A.coff[j];
            *base = (const uint8_t *)A.cig;
            *src = 4 * c0;
            *len = 4 * (A.coff[j + 1] - c0);
        } else {
            *src = R.rec + R.l_qname;
            *len = 4 * (int64_t)R.n_cigar;
        }
    } else if (k == 2) {
        *src = R.rec + R.l_qname + 4 * (int64_t)R.n_cigar;
        *len = (l + 1) / 2 + l;
    } else if (k < 3 + LFQ_BAM_MAX_KEEP) {
        const LfqBamPlan *P = A.plan + j;
        const int i = k - 3;
        if (i < P->n_keep) {
            *src = R.rec + P->keep_beg[i];
            *len = P->keep_len[i];
        } else {
            *src = 0;
            *len = 0;
        }
    } else {
        const int f = (k - 3 - LFQ_BAM_MAX_KEEP) / 3, part = (k - 3 - LFQ_BAM_MAX_KEEP) % 3;
        *src = 0;
        if (!((A.plan[j].append >> f) & 1u)) {
            *len = 0;
        } else if (part == 1) {
            *base = f == 0 ? A.lb : f == 1 ? A.ai : f == 2 ? A.ad : f == 3 ? A.bi : A.bd;
            *src = A.soff[j];
            *len = l;
        } else {
            *base = nullptr;
            *len = part == 0 ? 3 : 1;
            if (part == 0) {            /* tag, then the type Z */
                const uint32_t tag = f == 0 ? ('l' | 'b' << 8) : f == 1 ? ('a' | 'i' << 8) : f == 2 ? ('a' | 'd' << 8)
                                     : f == 3 ? ('B' | 'I' << 8) : ('B' | 'D' << 8);
                *cval = tag | ((uint32_t)'Z' << 16);
            }
        }
    }
}

__global__ __launch_bounds__(LFQ_BAM_COPY_CHUNKS) void lfq_bam_copy_kernel(LfqBamEncArgs A)
{
    const int64_t b0 = ((int64_t)blockIdx.x * LFQ_BAM_COPY_CHUNKS + threadIdx.x) * 16;
    if (b0 >= A.n_out) {
        return;
    }
    /* the chunk's first record: among those of the workgroup's tile (the host wrote down where each tile begins) */
    const int64_t r_lo = A.tile_rec[blockIdx.x], r_hi = blockIdx.x + 1 < gridDim.x ? A.tile_rec[blockIdx.x + 1] : A.n_reads - 1;
    int64_t j = bam_read_of_base(A.out_off, r_lo, r_hi, b0);
    const int total = (int)min((int64_t)16, A.n_out - b0);
    LfqBamRead R = A.reads[j];
    int64_t o = b0 - A.out_off[j];      /* where in record j the next byte comes from, and the segment that starts at seg0 */
    int64_t seg0 = 0;
    int k = 0, filled = 0;
    LfqB16 acc;
    acc.lo = acc.hi = 0;
    while (filled < total) {
        if (k == LFQ_BAM_N_SEGMENTS) {  /* on to the next record */
            j++;
            if (j >= A.n_reads) {
                break;
            }
            R = A.reads[j];
            k = 0;
            seg0 = 0;
            o = 0;
            continue;
        }
        const uint8_t *base;
        int64_t src, len;
        uint32_t cval;
        bam_enc_segment(A, j, R, k, &base, &src, &len, &cval);
        if (o >= seg0 + len) {
            seg0 += len;
            k++;
            continue;
        }
        const int64_t at = o - seg0;
        const int cnt = (int)min(len - at, (int64_t)(total - filled));
        LfqB16 v;
        if (base) {
            v = b16_fetch(base, src + at, cnt);
        } else {
            const LfqB16 m = b16_mask(cnt);
            v.lo = (uint64_t)(cval >> ((int)at * 8)) & m.lo;
            v.hi = 0;
        }
        v = b16_shl_bytes(v, filled);
        acc.lo |= v.lo;
        acc.hi |= v.hi;
        filled += cnt;
        o += cnt;
    }
    b16_store(A.out + b0, acc);
}

/* ---- host side of the encode's two launches ------------------------------------------------------------------------------------------ */
/* the context's result: n records in `data`, beside them what the state's vectors hold */
static int bam_publish(LfqBamState *S, int64_t n, const uint8_t *data, const lfq_bam_encoded **out)
{
    S->result.n_reads = n;
    S->result.data = data;
    S->result.data_off = S->data_off.data();
    S->result.src = S->src.data();
    S->result.pos = S->pos.data();
    S->result.n_cigar = S->n_cigar.data();
    *out = &S->result;
    return LFQ_OK;
}

int lfq_bam_encode_empty(lfq_ctx *c, const lfq_bam_encoded **out)
{
    LfqBamState *S = bam_state(c);
    S->enc_times = {};
    S->frame_live = 0;
    S->enc_lq.clear();
    S->enc_ls.clear();
    S->enc_live = true;                 /* (an empty result is a result) */
    S->data_off.assign(1, 0);
    S->src.assign(1, 0);
    S->pos.assign(1, 0);
    S->n_cigar.assign(1, 0);
    return bam_publish(S, 0, S->none, out);
}

/* records down, plan pass, lengths back, offsets down, copy pass, blob back.  Blocks. */
int lfq_bam_encode(lfq_ctx *c, const LfqBamEncIn *in, const lfq_bam_encoded **out)
{
    LfqBamState *S = bam_state(c);
    const int64_t n = in->n;
    S->enc_live = false;                /* the result before this one is gone, and the body framed from it */
    S->frame_live = 0;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    lfq_bam_encode_times &T = S->enc_times;
    T = {};
    T.n_reads = n;
    T.n_in_bytes = in->recs.data_bytes;
    const int64_t o_reads = lfq_al(in->recs.first_shift + in->recs.data_bytes + 16),
                  o_plan = o_reads + lfq_al(n * (int64_t)sizeof(LfqBamRead)), o_len = o_plan + lfq_al(n * (int64_t)sizeof(LfqBamPlan)),
                  o_err = o_len + lfq_al(n * 8), total = o_err + 256;
    LfqPin<int32_t> verdict(c, 4);
    LFQ_PIN_OK(verdict);
    LfqPin<int64_t> lens(c, (size_t)n);
    LFQ_PIN_OK(lens);
    LFQ_TRY(bam_upload(c, S, in->recs, total, o_reads, in->reads, (size_t)n * sizeof(LfqBamRead), o_err));
    hipStream_t st = c->stream;
    LfqBamEncArgs A;
    memset(&A, 0, sizeof(A));
    A.data = S->d_buf;
    A.reads = (const LfqBamRead *)(S->d_buf + o_reads);
    A.plan = (LfqBamPlan *)(S->d_buf + o_plan);
    A.out_len = (int64_t *)(S->d_buf + o_len);
    A.err = (int32_t *)(S->d_buf + o_err);
    A.coff = in->rd.cigar_off; A.soff = in->rd.seq_off; A.cig = in->rd.cigar; A.fl = in->d_fl;
    A.lb = in->d_lb; A.ai = in->d_ai; A.ad = in->d_ad; A.bi = in->d_bi; A.bd = in->d_bd;
    A.n_reads = n;
    A.what = in->what;
    A.uniform = in->uniform ? 1 : 0;
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bam_plan_kernel, dim3((unsigned)((n + LFQ_BAM_PLAN_READS - 1) / LFQ_BAM_PLAN_READS)),
                       dim3(LFQ_BAM_PLAN_READS), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    T.n_launches += 1;
    LFQ_TRY_HIP(hipMemcpyAsync(verdict.data(), A.err, 16, hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipMemcpyAsync(lens.data(), A.out_len, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bam_add_ms(S->up_t, &T.upload_ms));
    LFQ_TRY(bam_add_ms(S->kern_t, &T.kernels_ms));
    if (verdict[0]) {
        return LFQ_ERR_INVALID;
    }
    /* offsets in read-set order, and for every tile of the copy pass the record that holds its first byte */
    const int64_t tile = (int64_t)LFQ_BAM_COPY_CHUNKS * 16;
    S->data_off.resize((size_t)n + 1);
    S->data_off[0] = 0;
    for (int64_t j = 0; j < n; j++) {
        S->data_off[(size_t)j + 1] = S->data_off[(size_t)j] + lens[(size_t)j];
    }
    const int64_t n_out = S->data_off[(size_t)n], n_tiles = (n_out + tile - 1) / tile;
    LfqPin<int64_t> down(c, (size_t)(n + 1 + n_tiles));
    LFQ_PIN_OK(down);
    memcpy(down.data(), S->data_off.data(), (size_t)(n + 1) * 8);
    for (int64_t t = 0, j = 0; t < n_tiles; t++) {
        while (S->data_off[(size_t)j + 1] <= t * tile) {    /* (t * tile < n_out = data_off[n]: j stays below n) */
            j++;
        }
        down[(size_t)(n + 1 + t)] = j;
    }
    const int64_t o_off = 0, o_tile = lfq_al((n + 1) * 8), o_blob = o_tile + lfq_al(n_tiles * 8), out_total = o_blob + lfq_al(n_out + 16);
    LFQ_TRY(grow(&S->d_out, &S->d_out_bytes, out_total));
    if (n_out + 16 > S->h_out_bytes) {  /* a quarter over the need, as the staging area */
        LFQ_TRY(grow_pinned(&S->h_out, &S->h_out_bytes, std::max<int64_t>(n_out + n_out / 4 + 16, 1 << 16)));
    }
    if (n_out > 0) {
        A.out_off = (const int64_t *)(S->d_out + o_off);
        A.tile_rec = (const int64_t *)(S->d_out + o_tile);
        A.out = S->d_out + o_blob;
        A.n_out = n_out;
        LFQ_TRY(S->up_t.begin(st));
        LFQ_TRY_HIP(hipMemcpyAsync(S->d_out + o_off, down.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
        LFQ_TRY_HIP(hipMemcpyAsync(S->d_out + o_tile, down.data() + n + 1, (size_t)n_tiles * 8, hipMemcpyHostToDevice, st));
        LFQ_TRY(S->up_t.end(st));
        LFQ_TRY(S->kern_t.begin(st));
        hipLaunchKernelGGL(lfq_bam_copy_kernel, dim3((unsigned)n_tiles), dim3(LFQ_BAM_COPY_CHUNKS), 0, st, A);
        LFQ_TRY_HIP(hipGetLastError());
        LFQ_TRY(S->kern_t.end(st));
        T.n_launches += 1;
        LFQ_TRY(S->down_t.begin(st));
        LFQ_TRY_HIP(hipMemcpyAsync(S->h_out, A.out, (size_t)n_out, hipMemcpyDeviceToHost, st));
        LFQ_TRY(S->down_t.end(st));
        LFQ_TRY_HIP(hipStreamSynchronize(st));
        LFQ_TRY(bam_add_ms(S->up_t, &T.upload_ms));
        LFQ_TRY(bam_add_ms(S->kern_t, &T.kernels_ms));
        LFQ_TRY(bam_add_ms(S->down_t, &T.download_ms));
    }
    T.n_out_bytes = n_out;
    S->src.assign(in->src, in->src + n);
    S->pos.assign(in->pos, in->pos + n);
    S->n_cigar.assign(in->n_cigar, in->n_cigar + n);
    S->enc_lq.resize((size_t)n);
    S->enc_ls.resize((size_t)n);
    for (int64_t j = 0; j < n; j++) {
        S->enc_lq[(size_t)j] = in->reads[j].l_qname;
        S->enc_ls[(size_t)j] = in->reads[j].l_qseq;
    }
    S->enc_blob = o_blob;
    S->enc_live = n_out > 0;            /* (offsets and blob are on the device) */
    return bam_publish(S, n, S->h_out, out);
}

extern "C" int lfq_last_bam_encode_times(lfq_ctx *c, lfq_bam_encode_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = bam_state(c)->enc_times;
    return LFQ_OK;
}

/* ---- lfq_bam_frame_encoded: the body of a BAM file from the live encode result --------------------------------------------------- */
#define LFQ_BAM_FRAME_READS 256         /* reads per workgroup of the core pass: one lane each */
#define LFQ_BAM_FRAME_CHUNKS 256        /* 16-byte chunks of the body per workgroup of the gather pass: one lane each */
#define LFQ_BAM_FRAME_HEAD 36           /* block_size and the core, in front of every record */

struct LfqBamFrameArgs {
    const uint8_t *blob;                /* the encode result's records */
    const int64_t *out_off;             /* [n + 1] where they start in it */
    const uint32_t *cores;              /* [n_cores][8] the caller's */
    const int64_t *src;                 /* [n] */
    const int32_t *pos;                 /* [n] */
    const uint32_t *n_cigar;            /* [n] */
    uint32_t *new_cores;                /* [n][8] */
    uint8_t *body;                      /* 16-byte aligned, 16 bytes of slack */
    int64_t n_reads, n_body;
};

/* the SAM specification's reg2bin (section 5.3) for [beg, end) */
__device__ __forceinline__ uint32_t bam_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

/* core' of read j: the caller's core of record src[j] with pos, n_cigar_op and bin replaced */
__global__ __launch_bounds__(LFQ_BAM_FRAME_READS) void lfq_bam_frame_core_kernel(LfqBamFrameArgs A)
{
    const int64_t j = (int64_t)blockIdx.x * LFQ_BAM_FRAME_READS + threadIdx.x;
    if (j >= A.n_reads) {
        return;
    }
    const uint32_t *ci = A.cores + 8 * A.src[j];
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        w[k] = ci[k];
    }
    const uint32_t l_qname = w[2] & 0xffu, flag = w[3] >> 16, nc = A.n_cigar[j];
    /* the CIGAR words of the OUTPUT record: behind its name, inside the record (the host checked l_qname against it, and the
     * encode wrote n_cigar words there) */
    const int64_t rec = A.out_off[j], rec_end = A.out_off[j + 1];
    int64_t ref_bases = 0;
    for (uint32_t k = 0; k < nc; k++) {
        const int64_t at = rec + l_qname + 4 * (int64_t)k;
        if (at + 4 > rec_end) {
            break;
        }
        const uint32_t cw = (uint32_t)A.blob[at] | ((uint32_t)A.blob[at + 1] << 8) | ((uint32_t)A.blob[at + 2] << 16)
                            | ((uint32_t)A.blob[at + 3] << 24);
        const uint32_t op = cw & 0xfu;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) {
            ref_bases += cw >> 4;
        }
    }
    const int64_t pos = A.pos[j], end = pos + ((flag & 4u) || ref_bases == 0 ? 1 : ref_bases);
    w[1] = (uint32_t)A.pos[j];
    w[2] = (w[2] & 0xffffu) | (bam_reg2bin(pos, end) << 16);
    w[3] = (w[3] & 0xffff0000u) | (nc & 0xffffu);
    uint32_t *co = A.new_cores + 8 * j;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        co[k] = w[k];
    }
}

/* 16 bytes of the body per lane: record j starts at out_off[j] + 36 j and is block_size | core' | the record's bytes */
__global__ __launch_bounds__(LFQ_BAM_FRAME_CHUNKS) void lfq_bam_frame_gather_kernel(LfqBamFrameArgs A)
{
    const int64_t b0 = ((int64_t)blockIdx.x * LFQ_BAM_FRAME_CHUNKS + threadIdx.x) * 16;
    if (b0 >= A.n_body) {
        return;
    }
    int64_t lo = 0, hi = A.n_reads - 1;         /* the last record that starts at or in front of b0 */
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (A.out_off[mid] + LFQ_BAM_FRAME_HEAD * mid <= b0) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    int64_t j = lo, start = A.out_off[j] + LFQ_BAM_FRAME_HEAD * j, next = A.out_off[j + 1] + LFQ_BAM_FRAME_HEAD * (j + 1);
    uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int64_t p = b0 + k;
        if (p < A.n_body) {
            if (p >= next) {                    /* (a record is 36 bytes at least: one step a chunk at most; p < n_body keeps j < n) */
                j++;
                start = next;
                next = A.out_off[j + 1] + LFQ_BAM_FRAME_HEAD * (j + 1);
            }
            const int64_t o = p - start;
            uint32_t byte;
            if (o < 4) {
                byte = ((uint32_t)(A.out_off[j + 1] - A.out_off[j] + 32) >> (8 * (int)o)) & 0xffu;
            } else if (o < LFQ_BAM_FRAME_HEAD) {
                byte = (A.new_cores[8 * j + ((o - 4) >> 2)] >> (8 * (int)((o - 4) & 3))) & 0xffu;
            } else {
                byte = A.blob[A.out_off[j] + o - LFQ_BAM_FRAME_HEAD];
            }
            v[k >> 2] |= byte << (8 * (k & 3));
        }
    }
    uint32_t *dst = (uint32_t *)(A.body + b0);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        dst[k] = v[k];
    }
}

const uint8_t *lfq_bam_framed_resident(lfq_ctx *c, const uint8_t *p, int64_t bytes)
{
    LfqBamState *S = c->bam;
    if (!S || S->frame_live <= 0 || !p || bytes <= 0) {
        return nullptr;
    }
    const uint8_t *h = S->framed.data;
    if (p < h || p + bytes > h + S->frame_live) {
        return nullptr;
    }
    return S->d_frame + S->frame_body + (p - h);
}

extern "C" int lfq_bam_frame_encoded(lfq_ctx *c, const uint8_t *cores, int64_t n_cores, const lfq_bam_framed **out)
{
    if (out) *out = nullptr;
    if (!c || !cores || !out || n_cores < 0) {
        return LFQ_ERR_INVALID;
    }
    LfqBamState *S = c->bam;
    if (!S || !S->enc_live) {
        return LFQ_ERR_INVALID;
    }
    const int64_t n = S->result.n_reads;
    for (int64_t j = 0; j < n; j++) {
        const int64_t s = S->src[(size_t)j];
        if (s < 0 || s >= n_cores) {
            return LFQ_ERR_INVALID;
        }
        const uint8_t *co = cores + 32 * s;
        int32_t l_seq;
        memcpy(&l_seq, co + 16, 4);
        if (co[8] != S->enc_lq[(size_t)j] || l_seq != S->enc_ls[(size_t)j] || S->n_cigar[(size_t)j] > 0xffffu) {
            return LFQ_ERR_INVALID;
        }
    }
    S->frame_live = 0;                  /* the body before this one is gone */
    S->rec_off.resize((size_t)n + 1);
    for (int64_t j = 0; j <= n; j++) {
        S->rec_off[(size_t)j] = S->data_off[(size_t)j] + LFQ_BAM_FRAME_HEAD * j;
    }
    lfq_bam_framed &F = S->framed;
    F.n_reads = n;
    F.rec_off = S->rec_off.data();
    F.data = S->none;
    F.n_bytes = S->rec_off[(size_t)n];
    if (n == 0) {
        *out = &F;
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    const int64_t n_body = F.n_bytes;
    const int64_t o_src = lfq_al(n_cores * 32), o_pos = o_src + lfq_al(n * 8), o_nc = o_pos + lfq_al(n * 4), o_new = o_nc + lfq_al(n * 4),
                  o_body = o_new + lfq_al(n * 32), total = o_body + lfq_al(n_body + 16);
    LFQ_TRY(grow(&S->d_frame, &S->d_frame_bytes, total));
    if (n_body + 16 > S->h_frame_bytes) {
        LFQ_TRY(grow_pinned(&S->h_frame, &S->h_frame_bytes, std::max<int64_t>(n_body + n_body / 4 + 16, 1 << 16)));
    }
    /* one pinned block down: cores | src | pos | n_cigar, laid out as on the device */
    LfqPin<uint8_t> down(c, (size_t)o_new);
    LFQ_PIN_OK(down);
    memcpy(down.data(), cores, (size_t)n_cores * 32);
    memcpy(down.data() + o_src, S->src.data(), (size_t)n * 8);
    memcpy(down.data() + o_pos, S->pos.data(), (size_t)n * 4);
    memcpy(down.data() + o_nc, S->n_cigar.data(), (size_t)n * 4);
    hipStream_t st = c->stream;
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_frame, down.data(), (size_t)o_new, hipMemcpyHostToDevice, st));
    LfqBamFrameArgs A;
    A.blob = S->d_out + S->enc_blob;
    A.out_off = (const int64_t *)S->d_out;
    A.cores = (const uint32_t *)S->d_frame;
    A.src = (const int64_t *)(S->d_frame + o_src);
    A.pos = (const int32_t *)(S->d_frame + o_pos);
    A.n_cigar = (const uint32_t *)(S->d_frame + o_nc);
    A.new_cores = (uint32_t *)(S->d_frame + o_new);
    A.body = S->d_frame + o_body;
    A.n_reads = n;
    A.n_body = n_body;
    hipLaunchKernelGGL(lfq_bam_frame_core_kernel, dim3((unsigned)((n + LFQ_BAM_FRAME_READS - 1) / LFQ_BAM_FRAME_READS)),
                       dim3(LFQ_BAM_FRAME_READS), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    const int64_t n_chunks = (n_body + 15) / 16;
    hipLaunchKernelGGL(lfq_bam_frame_gather_kernel, dim3((unsigned)((n_chunks + LFQ_BAM_FRAME_CHUNKS - 1) / LFQ_BAM_FRAME_CHUNKS)),
                       dim3(LFQ_BAM_FRAME_CHUNKS), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY_HIP(hipMemcpyAsync(S->h_frame, A.body, (size_t)n_body, hipMemcpyDeviceToHost, st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    S->frame_body = o_body;
    S->frame_live = n_body;
    F.data = S->h_frame;
    *out = &F;
    return LFQ_OK;
}
