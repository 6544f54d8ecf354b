/*
 * lfq_bgzf.hip -- BGZF blocks inflated on the device (lfq_bgzf_inflate), the record scan behind them
 * (lfq_bam_scan_records, host only) and the entry that chains both into the BAM decode (lfq_readset_create_from_bgzf).
 *
 * The kernel runs lfq_inflate.h, one wavefront per block.  Every lane of the wavefront walks the symbols -- the same bits, the same
 * tables, the same branches: the walk is serial and costs a wavefront what it costs a lane -- and what a symbol produces is cut
 * over the lanes: up to 64 pending literals are one store, a match or a stored block is a 64-byte-wide copy, a table is filled 64
 * entries a trip.  A block's output (at most 64 KiB) is staged in LDS, where a back-reference is an LDS read, and goes to global
 * memory once, as aligned dwords, after its CRC-32 has been checked: LFQ_BGZF_BLOCKS_PER_WG x (64 KiB + 5.8 KiB of tables) of the
 * 160 KiB.
 */
#include <memory>

#include "lfq_ctx.h"
#include "lfq_inflate.h"

#define LFQ_BGZF_BLOCKS_PER_WG 2        /* wavefronts, and staged blocks, per workgroup */

struct LfqBgzfBlock {                   /* per block, from the host's header walk */
    int64_t in_beg, in_end;             /* the deflate stream in the compressed bytes: behind the header, in front of the trailer */
    int64_t out_off;                    /* prefix sum of ISIZE */
    uint32_t isize, crc;                /* the trailer */
};

struct LfqBgzfArgs {
    const uint8_t *comp;                /* 4-byte aligned, 16 bytes of slack behind the last block */
    const LfqBgzfBlock *blocks;
    int32_t *status;                    /* [n_blocks] */
    uint8_t *out;                       /* 16 bytes of slack */
    int64_t n_blocks;
};

/* what one worker stored to LDS is what the others load: LDS serves a wavefront's instructions in order, the fence keeps the
 * compiler from moving them */
__device__ __forceinline__ void bgzf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* the staged output is addressed as LDS (a generic pointer would make every access a flat one); volatile: a lane loads what another
 * lane of its wavefront stored an instruction earlier */
typedef __attribute__((address_space(3))) volatile uint8_t LfqLdsU8;
typedef __attribute__((address_space(3))) volatile uint32_t LfqLdsU32;

/* lfq_inflate.h's Io on the device */
struct LfqInfDevIo {
    const uint8_t *comp;
    int64_t d_lo, d_hi;                 /* the aligned dwords that hold the block's first and last compressed byte */
    LfqLdsU8 *out;                      /* LFQ_INF_MAX_OUT bytes */
    int ln;
    /* the input window: lane i holds dword w0 + i; `nxt` is the window behind it, loaded when this one was taken */
    int64_t w0, nw0;
    uint32_t win, nxt;
    /* literals not stored yet: lane i holds the i-th of npend, the first one belongs at pend_at */
    uint32_t pend, pend_at;
    int npend;

    __device__ __forceinline__ uint32_t load_dword(int64_t d) const
    {
        return d >= d_lo && d <= d_hi ? ((const uint32_t *)comp)[d] : 0u;
    }
    __device__ __forceinline__ uint32_t dword_at(int64_t d)
    {
        if (d < w0 || d >= w0 + 64) {
            win = d == nw0 ? nxt : load_dword(d + ln);
            w0 = d;
            nw0 = d + 64;
            nxt = load_dword(nw0 + ln);
        }
        return (uint32_t)__builtin_amdgcn_readlane((int)win, (int)(d - w0));
    }
    __device__ __forceinline__ uint32_t in8(int64_t p) { return (dword_at(p >> 2) >> ((int)(p & 3) * 8)) & 0xffu; }
    __device__ __forceinline__ uint32_t in32(int64_t p)
    {
        const uint32_t lo = dword_at(p >> 2);
        const int sh = (int)(p & 3) * 8;
        if (!sh) {
            return lo;
        }
        const uint32_t hi = dword_at((p >> 2) + 1);
        return (lo >> sh) | (hi << (32 - sh));
    }
    __device__ __forceinline__ void flush()
    {
        if (ln < npend) {
            out[pend_at + ln] = (uint8_t)pend;
        }
        npend = 0;
    }
    __device__ __forceinline__ void lit(uint32_t at, uint32_t v)
    {
        if (npend == 0) {
            pend_at = at;
        }
        if (ln == npend) {
            pend = v;
        }
        npend++;
        if (npend == 64) {
            flush();
        }
    }
    __device__ __forceinline__ void match(uint32_t at, uint32_t dist, uint32_t len)
    {
        flush();
        bgzf_wave_sync();
        /* byte k of the match is byte k mod dist of the dist bytes in front of it, all of them written: a byte-by-byte copy */
        for (uint32_t k = (uint32_t)ln; k < len; k += 64) {
            const uint32_t s = dist >= len ? k : dist == 1 ? 0u : k % dist;
            out[at + k] = out[at - dist + s];
        }
    }
    __device__ __forceinline__ void stored(uint32_t at, int64_t p, uint32_t len)
    {
        flush();
        for (uint32_t k = (uint32_t)ln; k < len; k += 64) {
            out[at + k] = comp[p + k];
        }
    }
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ void sync() { bgzf_wave_sync(); }
};

__global__ __launch_bounds__(64 * LFQ_BGZF_BLOCKS_PER_WG) void lfq_bgzf_inflate_kernel(LfqBgzfArgs A)
{
    __shared__ uint32_t s_out[LFQ_BGZF_BLOCKS_PER_WG][LFQ_INF_MAX_OUT / 4];
    __shared__ LfqInfTables s_tab[LFQ_BGZF_BLOCKS_PER_WG];
    __shared__ uint32_t s_crc[256];
    for (uint32_t i = threadIdx.x; i < 256; i += 64 * LFQ_BGZF_BLOCKS_PER_WG) {
        s_crc[i] = lfq_crc_table_entry(i);
    }
    __syncthreads();                    /* the only workgroup barrier: from here on a wavefront is on its own */
    const int wave = (int)(threadIdx.x >> 6), ln = (int)(threadIdx.x & 63);
    const int64_t b = (int64_t)blockIdx.x * LFQ_BGZF_BLOCKS_PER_WG + wave;
    if (b >= A.n_blocks) {
        return;
    }
    const LfqBgzfBlock blk = A.blocks[b];
    LfqInfDevIo io;
    io.comp = A.comp;
    io.d_lo = blk.in_beg >> 2;
    io.d_hi = blk.in_end > blk.in_beg ? (blk.in_end - 1) >> 2 : io.d_lo - 1;
    io.out = (LfqLdsU8 *)s_out[wave];
    io.ln = ln;
    io.w0 = io.nw0 = -((int64_t)1 << 40);   /* no window yet */
    io.win = io.nxt = 0;
    io.pend = io.pend_at = 0;
    io.npend = 0;
    uint32_t n_out = 0;
    int st = lfq_inflate(&s_tab[wave], blk.in_beg, blk.in_end, blk.isize, &n_out, io);
    io.flush();
    bgzf_wave_sync();
    /* CRC-32: a slice of whole dwords per lane, then each slice's CRC times x^(8 * bytes behind it), summed over the lanes */
    const uint32_t n = n_out, each = lfq_crc_slice_bytes(n);
    const uint32_t a = min((uint32_t)ln * each, n), e = min(a + each, n);
    uint32_t crc = 0xffffffffu;
    LfqLdsU32 *o32 = (LfqLdsU32 *)s_out[wave];
    uint32_t i = a;
    for (; i + 4 <= e; i += 4) {
        uint32_t w = o32[i >> 2];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            crc = s_crc[(crc ^ w) & 0xffu] ^ (crc >> 8);
            w >>= 8;
        }
    }
    for (; i < e; i++) {
        crc = s_crc[(crc ^ io.out[i]) & 0xffu] ^ (crc >> 8);
    }
    crc = e > a ? ~crc : 0u;
    crc = lfq_crc_mul(lfq_crc_x8n(n - e), crc);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        crc ^= (uint32_t)__shfl_xor((int)crc, m, 64);
    }
    if (st == LFQ_INF_OK && crc != blk.crc) {
        st = LFQ_INF_CRC;
    }
    if (ln == 0) {
        A.status[b] = st;
    }
    if (st != LFQ_INF_OK) {
        return;
    }
    /* LDS -> [out_off, out_off + ISIZE): bytes up to the first aligned dword, dwords, the bytes behind the last one */
    uint8_t *g = A.out + blk.out_off;
    const uint32_t head = min(n, (uint32_t)((4 - ((uintptr_t)g & 3)) & 3)), nd = (n - head) >> 2, tail = head + 4 * nd;
    if ((uint32_t)ln < head) {
        g[ln] = io.out[ln];
    }
    const int sh = (int)(head & 3) * 8;
    for (uint32_t j = (uint32_t)ln; j < nd; j += 64) {
        const uint32_t o = head + 4 * j;
        uint32_t w = o32[o >> 2];
        if (sh) {                       /* (o + 3 < n: the dword behind holds a byte of the output) */
            w = (w >> sh) | (o32[(o >> 2) + 1] << (32 - sh));
        }
        *(uint32_t *)(g + o) = w;
    }
    if (tail + (uint32_t)ln < n) {
        g[tail + ln] = io.out[tail + ln];
    }
}

/* ---- host side ------------------------------------------------------------------------------------------------------------------- */
struct LfqBgzfState {
    uint8_t *d_buf = nullptr;           /* compressed bytes | block descriptors | statuses (grow-only) */
    int64_t d_bytes = 0;
    uint8_t *d_out = nullptr;           /* the inflated bytes: resident until the next inflate (grow-only) */
    int64_t d_out_bytes = 0;
    uint8_t *h_stage = nullptr;         /* pinned staging of compressed bytes that come in pageable memory (grow-only) */
    int64_t h_stage_bytes = 0;
    uint8_t *h_out = nullptr;           /* statuses | the inflated bytes on the host, pinned (grow-only) */
    int64_t h_out_bytes = 0;
    int64_t live_bytes = 0;             /* bytes of the live result in d_out / at result.data; 0: none */
    std::vector<int64_t> comp_off, data_off;
    int32_t none_status[4] = {};
    uint8_t none[16] = {};
    lfq_bgzf_result result = {};
    lfq_bgzf_times times = {};
    LfqEvPair up_t = {}, kern_t = {}, down_t = {};
};

static LfqBgzfState *bgzf_state(lfq_ctx *c)
{
    if (!c->bgzf) {
        c->bgzf = new LfqBgzfState();
    }
    return c->bgzf;
}

void lfq_bgzf_release(lfq_ctx *c)
{
    if (LfqBgzfState *S = c->bgzf) {
        if (S->d_buf) (void)hipFree(S->d_buf);
        if (S->d_out) (void)hipFree(S->d_out);
        free_pinned(&S->h_stage, &S->h_stage_bytes);
        free_pinned(&S->h_out, &S->h_out_bytes);
        for (LfqEvPair *t : {&S->up_t, &S->kern_t, &S->down_t}) {
            t->destroy();
        }
        delete S;
        c->bgzf = nullptr;
    }
}

const uint8_t *lfq_bgzf_resident_bytes(lfq_ctx *c, const uint8_t *p, int64_t bytes)
{
    LfqBgzfState *S = c->bgzf;
    if (!S || S->live_bytes <= 0 || !p || bytes <= 0) {
        return nullptr;
    }
    const uint8_t *h = S->result.data;
    if (p < h || p + bytes > h + S->live_bytes) {
        return nullptr;
    }
    return S->d_out + (p - h);
}

const uint8_t *lfq_bgzf_resident(lfq_ctx *c, const uint8_t *p, int64_t bytes)
{
    const uint8_t *d = lfq_bgzf_resident_bytes(c, p, bytes);
    if (d) {
        c->bgzf->times.n_decodes_from_device += 1;
    }
    return d;
}

static inline uint32_t bgzf_le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static inline uint32_t bgzf_le32(const uint8_t *p) { return bgzf_le16(p) | (bgzf_le16(p + 2) << 16); }

/* the header walk (SAM specification section 4.1): blocks[] and the two offset arrays, or LFQ_ERR_INVALID */
static int bgzf_walk(const uint8_t *comp, int64_t n, std::vector<LfqBgzfBlock> *blocks, std::vector<int64_t> *comp_off,
                     std::vector<int64_t> *data_off)
{
    comp_off->assign(1, 0);
    data_off->assign(1, 0);
    blocks->clear();
    int64_t p = 0;
    while (p < n) {
        if (n - p < 12) {
            return LFQ_ERR_INVALID;
        }
        const uint8_t *h = comp + p;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) {
            return LFQ_ERR_INVALID;
        }
        const int64_t xlen = bgzf_le16(h + 10), x0 = p + 12, x1 = x0 + xlen;
        if (x1 > n) {
            return LFQ_ERR_INVALID;
        }
        int64_t bsize = -1;
        for (int64_t q = x0; q < x1;) {             /* a subfield a trip: four bytes at least */
            if (x1 - q < 4) {
                return LFQ_ERR_INVALID;
            }
            const int64_t slen = bgzf_le16(comp + q + 2);
            if (slen > x1 - q - 4) {
                return LFQ_ERR_INVALID;
            }
            if (bsize < 0 && comp[q] == 'B' && comp[q + 1] == 'C' && slen == 2) {
                bsize = (int64_t)bgzf_le16(comp + q + 4) + 1;
            }
            q += 4 + slen;
        }
        if (bsize < 0 || bsize < 12 + xlen + 8 || bsize > n - p) {
            return LFQ_ERR_INVALID;
        }
        LfqBgzfBlock B;
        B.in_beg = x1;
        B.in_end = p + bsize - 8;
        B.crc = bgzf_le32(comp + p + bsize - 8);
        B.isize = bgzf_le32(comp + p + bsize - 4);
        if (B.isize > LFQ_INF_MAX_OUT) {
            return LFQ_ERR_INVALID;
        }
        B.out_off = data_off->back();
        blocks->push_back(B);
        p += bsize;
        comp_off->push_back(p);
        data_off->push_back(B.out_off + B.isize);
    }
    return LFQ_OK;
}

extern "C" int lfq_bgzf_inflate(lfq_ctx *c, const uint8_t *comp, int64_t n_bytes, const lfq_bgzf_result **out)
{
    if (out) *out = nullptr;
    if (!c || !out || n_bytes < 0 || (n_bytes > 0 && !comp)) {
        return LFQ_ERR_INVALID;
    }
    std::vector<LfqBgzfBlock> blocks;
    std::vector<int64_t> comp_off, data_off;
    LFQ_TRY(bgzf_walk(comp, n_bytes, &blocks, &comp_off, &data_off));
    LfqBgzfState *S = bgzf_state(c);
    const int64_t nb = (int64_t)blocks.size(), n_out = data_off.back();
    S->live_bytes = 0;                  /* the result before this one is gone */
    S->comp_off.swap(comp_off);
    S->data_off.swap(data_off);
    S->times = {};
    S->times.n_blocks = nb;
    S->times.n_in_bytes = n_bytes;
    S->times.n_out_bytes = n_out;
    lfq_bgzf_result &R = S->result;
    R.n_blocks = nb;
    R.comp_off = S->comp_off.data();
    R.data_off = S->data_off.data();
    R.status = S->none_status;
    R.data = S->none;
    R.n_bytes = n_out;
    if (nb == 0) {
        *out = &R;
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    const int64_t o_desc = lfq_al(n_bytes + 16), o_status = o_desc + lfq_al(nb * (int64_t)sizeof(LfqBgzfBlock)),
                  total = o_status + lfq_al(nb * 4);
    const int64_t h_data = lfq_al(nb * 4);
    LFQ_TRY(grow(&S->d_buf, &S->d_bytes, total));
    LFQ_TRY(grow(&S->d_out, &S->d_out_bytes, lfq_al(n_out + 16)));
    if (h_data + n_out + 16 > S->h_out_bytes) {
        LFQ_TRY(grow_pinned(&S->h_out, &S->h_out_bytes, h_data + n_out + n_out / 4 + 16));
    }
    LfqPin<LfqBgzfBlock> desc(c, (size_t)nb);
    LFQ_PIN_OK(desc);
    memcpy(desc.data(), blocks.data(), (size_t)nb * sizeof(LfqBgzfBlock));
    const uint8_t *src = comp;
    if (!lfq_is_pinned(comp)) {
        if (n_bytes > S->h_stage_bytes) {
            LFQ_TRY(grow_pinned(&S->h_stage, &S->h_stage_bytes, std::max<int64_t>(n_bytes + n_bytes / 4, 1 << 16)));
        }
        memcpy(S->h_stage, comp, (size_t)n_bytes);
        src = S->h_stage;
    }
    hipStream_t st = c->stream;
    LFQ_TRY(S->up_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf, src, (size_t)n_bytes, hipMemcpyHostToDevice, st));
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf + o_desc, desc.data(), (size_t)nb * sizeof(LfqBgzfBlock), hipMemcpyHostToDevice, st));
    LFQ_TRY(S->up_t.end(st));
    LfqBgzfArgs A;
    A.comp = S->d_buf;
    A.blocks = (const LfqBgzfBlock *)(S->d_buf + o_desc);
    A.status = (int32_t *)(S->d_buf + o_status);
    A.out = S->d_out;
    A.n_blocks = nb;
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bgzf_inflate_kernel, dim3((unsigned)((nb + LFQ_BGZF_BLOCKS_PER_WG - 1) / LFQ_BGZF_BLOCKS_PER_WG)),
                       dim3(64 * LFQ_BGZF_BLOCKS_PER_WG), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    S->times.n_launches = 1;
    LFQ_TRY(S->down_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(S->h_out, A.status, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    if (n_out > 0) {
        LFQ_TRY_HIP(hipMemcpyAsync(S->h_out + h_data, S->d_out, (size_t)n_out, hipMemcpyDeviceToHost, st));
    }
    LFQ_TRY(S->down_t.end(st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(S->up_t.ms(&S->times.upload_ms));
    LFQ_TRY(S->kern_t.ms(&S->times.kernels_ms));
    LFQ_TRY(S->down_t.ms(&S->times.download_ms));
    R.status = (const int32_t *)S->h_out;
    R.data = S->h_out + h_data;
    *out = &R;
    for (int64_t b = 0; b < nb; b++) {
        if (R.status[b] != 0) {
            return LFQ_ERR_INVALID;     /* (nothing of this result is handed to a decode from the device) */
        }
    }
    S->live_bytes = n_out;
    return LFQ_OK;
}

extern "C" int lfq_last_bgzf_times(lfq_ctx *c, lfq_bgzf_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = bgzf_state(c)->times;
    return LFQ_OK;
}

/* ---- the record scan: sam_itr_next + mplp_func's filters over inflated bytes (include/lofreq_amd.h has the rules) ----------- */
struct LfqBamScanOwned {
    lfq_bam_scan pub;                   /* first: the pointer handed out is this struct's */
    std::vector<int64_t> data_off, data_end;
    std::vector<int32_t> pos, l_qseq;
    std::vector<uint16_t> flag, l_qname;
    std::vector<uint8_t> mapq;
    std::vector<uint32_t> n_cigar;
};

extern "C" void lfq_bam_scan_opts_init(lfq_bam_scan_opts *o)
{
    if (o) {
        o->tid = -1;
        o->beg = 0;
        o->end = INT64_MAX;
        o->min_mq = 0;
        o->max_mq = 255;
        o->no_orphan = 0;
        o->flag_mask = 4u | 256u | 512u | 1024u;
    }
}

extern "C" void lfq_bam_scan_free(lfq_bam_scan *s)
{
    delete (LfqBamScanOwned *)s;
}

extern "C" int lfq_bam_scan_records(const uint8_t *bam, int64_t first, int64_t stop, const lfq_bam_scan_opts *o, lfq_bam_scan **out)
{
    if (out) *out = nullptr;
    if (!bam || !o || !out || first < 0 || stop < first) {
        return LFQ_ERR_INVALID;
    }
    std::unique_ptr<LfqBamScanOwned> S(new LfqBamScanOwned());
    int64_t p = first, n_seen = 0, last_end = first;
    while (stop - p >= 4) {                         /* a record a trip: p grows by 36 at least */
        const int64_t bs = (int32_t)bgzf_le32(bam + p);
        if (bs < 32) {
            return LFQ_ERR_INVALID;
        }
        if (bs > stop - p - 4) {
            break;                                  /* the chunk ends inside this record */
        }
        const uint8_t *core = bam + p + 4;
        const int32_t ref_id = (int32_t)bgzf_le32(core), pos = (int32_t)bgzf_le32(core + 4), l_seq = (int32_t)bgzf_le32(core + 16);
        const uint32_t l_name = core[8], n_cig = bgzf_le16(core + 12), flag = bgzf_le16(core + 14);
        uint32_t mapq = core[9];
        if (l_seq < 0 || (int64_t)l_name + 4 * (int64_t)n_cig + ((int64_t)l_seq + 1) / 2 + l_seq > bs - 32) {
            return LFQ_ERR_INVALID;
        }
        n_seen++;
        const int64_t name_at = p + 36, rec_end = p + 4 + bs;
        p = rec_end;
        if (ref_id < 0 || (o->tid >= 0 && ref_id != o->tid) || (flag & o->flag_mask)) {
            continue;
        }
        int64_t ref_bases = 0;
        const uint8_t *cg = bam + name_at + l_name;
        for (uint32_t k = 0; k < n_cig; k++) {
            const uint32_t w = bgzf_le32(cg + 4 * (int64_t)k), op = w & 0xf;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) {
                ref_bases += w >> 4;
            }
        }
        const int64_t endpos = (int64_t)pos + (ref_bases ? ref_bases : 1);
        if (!((int64_t)pos < o->end && endpos > o->beg)) {
            continue;
        }
        if ((int64_t)mapq > o->max_mq) {            /* plp.c:707-721, the else-if chain */
            mapq = (uint32_t)std::max(o->max_mq, 0);
        } else if ((int64_t)mapq < o->min_mq) {
            continue;
        } else if (o->no_orphan && (flag & 1u) && !(flag & 2u)) {
            continue;
        }
        if (l_seq == 0 || n_cig == 0) {
            continue;
        }
        S->data_off.push_back(name_at);
        S->data_end.push_back(rec_end);
        S->pos.push_back(pos);
        S->flag.push_back((uint16_t)flag);
        S->mapq.push_back((uint8_t)mapq);
        S->l_qname.push_back((uint16_t)l_name);
        S->n_cigar.push_back(n_cig);
        S->l_qseq.push_back(l_seq);
        last_end = rec_end;
    }
    const int64_t n = (int64_t)S->pos.size();
    S->data_off.push_back(n ? last_end : first);
    if (n == 0) {                                   /* (no null arrays, whatever n) */
        S->data_end.push_back(first);
        S->pos.push_back(0); S->flag.push_back(0); S->mapq.push_back(0); S->l_qname.push_back(0); S->n_cigar.push_back(0);
        S->l_qseq.push_back(0);
    }
    memset(&S->pub, 0, sizeof(S->pub));
    S->pub.recs.n_reads = n;
    S->pub.recs.data = bam;
    S->pub.recs.data_off = S->data_off.data();
    S->pub.recs.pos = S->pos.data();
    S->pub.recs.flag = S->flag.data();
    S->pub.recs.mapq = S->mapq.data();
    S->pub.recs.l_qname = S->l_qname.data();
    S->pub.recs.n_cigar = S->n_cigar.data();
    S->pub.recs.l_qseq = S->l_qseq.data();
    S->pub.data_end = S->data_end.data();
    S->pub.n_seen = n_seen;
    S->pub.n_consumed = p;
    *out = &S.release()->pub;
    return LFQ_OK;
}

extern "C" int lfq_readset_create_from_bam_scan(lfq_ctx *c, const lfq_bam_scan *scan, unsigned read_tags, lfq_readset **out)
{
    if (out) *out = nullptr;
    if (!c || !scan || !out || (scan->recs.n_reads > 0 && !scan->data_end)) {
        return LFQ_ERR_INVALID;
    }
    return lfq_readset_from_bam_ends(c, &scan->recs, scan->data_end, read_tags, out);
}

extern "C" int lfq_readset_create_from_bgzf(lfq_ctx *c, const uint8_t *comp, int64_t n_bytes, int64_t first, int64_t stop_or_neg,
                                            const lfq_bam_scan_opts *o, const char *ref, int64_t ref_len, unsigned read_tags,
                                            lfq_readset **out, int64_t *n_consumed)
{
    if (out) *out = nullptr;
    if (!c || !out || !o || !ref) {
        return LFQ_ERR_INVALID;
    }
    const lfq_bgzf_result *R = nullptr;
    LFQ_TRY(lfq_bgzf_inflate(c, comp, n_bytes, &R));
    const int64_t stop = stop_or_neg < 0 ? R->n_bytes : stop_or_neg;
    if (first > R->n_bytes || stop > R->n_bytes) {
        return LFQ_ERR_INVALID;
    }
    lfq_bam_scan *scan = nullptr;
    LFQ_TRY(lfq_bam_scan_records(R->data, first, stop, o, &scan));
    scan->recs.ref = ref;
    scan->recs.ref_len = ref_len;
    if (n_consumed) {
        *n_consumed = scan->n_consumed;
    }
    const int rc = lfq_readset_create_from_bam_scan(c, scan, read_tags, out);
    lfq_bam_scan_free(scan);
    return rc;
}
