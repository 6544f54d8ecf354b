/*
 * lfq_bgzf_deflate.hip -- bytes cut into BGZF blocks and compressed on the device (lfq_bgzf_deflate): the way
 * out that mirrors lfq_bgzf.hip's way in.
 *
 * The first kernel runs lfq_deflate.h, one wavefront per block.  The block's payload (at most 65280 bytes) is staged in LDS, where
 * the hash table of the match search, the symbol counts, the codes and the bit window live beside it: LFQ_BGZF_DEF_BLOCKS_PER_WG x
 * (64 KiB + 13 KiB) of the 160 KiB.  That leaves no room for a second 64 KiB of output or for a token array, so the match pass runs
 * twice -- once to count the symbols, once to write them with the codes chosen -- and the stream goes to a slot of the block's own
 * in global memory as it is produced, full dwords at a time (DESIGN.md section 8 says why not a token scratch).  The CRC-32 of the
 * payload is computed from LDS with the sliced scheme of the inflate kernel.  Eight bytes a block, the stream's length and type, go
 * to the host, which makes comp_off of them; the second kernel then writes header, stream and trailer of every block to their
 * final, arbitrarily aligned places as aligned dwords, and one copy brings the blocks back.
 */
#include "lfq_ctx.h"
#include "lfq_deflate.h"

#define LFQ_BGZF_DEF_BLOCKS_PER_WG 2    /* wavefronts, and staged payloads, per workgroup */
#define LFQ_BGZF_PACK_THREADS 256
#define LFQ_BGZF_HEAD 18                /* bytes in front of a block's stream, and behind it */
#define LFQ_BGZF_TAIL 8

struct LfqDefArgs {
    const uint8_t *data;                /* byte 0 of the input on the device; the aligned dwords around its ends are the library's */
    const int64_t *data_off;            /* [n_blocks + 1] */
    uint8_t *slots;                     /* block b's stream: at lfq_def_slot_off(data_off[b], b), 5 + n_b bytes rounded up to dwords */
    LfqDefResult *res;                  /* [n_blocks] */
    uint32_t *crc;                      /* [n_blocks] */
    int64_t n_blocks;
    /* the second kernel */
    const int64_t *comp_off;            /* [n_blocks + 1] */
    uint32_t *comp;                     /* comp_off[n_blocks] bytes, rounded up to dwords */
};

/* slots abut: 4-byte aligned, and 12 bytes a block cover the 5 bytes of a stored block's header and the rounding at both ends */
__host__ __device__ static inline int64_t lfq_def_slot_off(int64_t data_off, int64_t b)
{
    return ((data_off + 3) & ~(int64_t)3) + 12 * b;
}

/* (as lfq_bgzf.hip's: LDS serves a wavefront's instructions in order, the fences keep the compiler from moving them) */
__device__ __forceinline__ void def_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef __attribute__((address_space(3))) const uint8_t LfqDefLdsU8;
typedef __attribute__((address_space(3))) const uint32_t LfqDefLdsU32;

/* lfq_deflate.h's Io on the device */
struct LfqDefDevIo {
    LfqDefLdsU32 *pay;                  /* the payload from LDS byte 0 on, a dword of room behind it */
    uint32_t *slot;
    uint32_t slot_dwords;
    int ln;
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ void sync() { def_wave_sync(); }
    __device__ __forceinline__ bool any(bool v) { return __builtin_amdgcn_ballot_w64(v) != 0; }
    __device__ __forceinline__ uint32_t ld8(uint32_t p) { return ((LfqDefLdsU8 *)pay)[p]; }
    __device__ __forceinline__ uint32_t ld32(uint32_t p)
    {
        const uint64_t two = (uint64_t)pay[p >> 2] | ((uint64_t)pay[(p >> 2) + 1] << 32);
        return (uint32_t)(two >> ((p & 3u) * 8u));
    }
    __device__ __forceinline__ void out32(uint32_t w, uint32_t v)
    {
        if (w < slot_dwords) {          /* (always: the stream chosen is at most 5 + n bytes) */
            slot[w] = v;
        }
    }
    __device__ __forceinline__ void add32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    __device__ __forceinline__ void or32(uint32_t *p, uint32_t v) { atomicOr(p, v); }
};

__global__ __launch_bounds__(64 * LFQ_BGZF_DEF_BLOCKS_PER_WG) void lfq_bgzf_deflate_kernel(LfqDefArgs A)
{
    __shared__ uint32_t s_pay[LFQ_BGZF_DEF_BLOCKS_PER_WG][LFQ_DEF_MAX_IN / 4 + 2];
    __shared__ LfqDefState s_st[LFQ_BGZF_DEF_BLOCKS_PER_WG];
    __shared__ uint32_t s_crc[256];
    for (uint32_t i = threadIdx.x; i < 256; i += 64 * LFQ_BGZF_DEF_BLOCKS_PER_WG) {
        s_crc[i] = lfq_crc_table_entry(i);
    }
    __syncthreads();                    /* the only workgroup barrier: from here on a wavefront is on its own */
    const int wave = (int)(threadIdx.x >> 6), ln = (int)(threadIdx.x & 63);
    const int64_t b = (int64_t)blockIdx.x * LFQ_BGZF_DEF_BLOCKS_PER_WG + wave;
    if (b >= A.n_blocks) {
        return;
    }
    const int64_t off = A.data_off[b], len64 = A.data_off[b + 1] - off;
    if (len64 <= 0 || len64 > LFQ_DEF_MAX_IN) {         /* (the host checked) */
        return;
    }
    const uint32_t n = (uint32_t)len64, nd = (n + 3) >> 2;
    /* global -> LDS: the aligned dwords that hold the payload, and no others, shifted so that payload byte 0 is LDS byte 0 */
    {
        const uintptr_t a = (uintptr_t)(A.data + off);
        const uint32_t *g32 = (const uint32_t *)(a & ~(uintptr_t)3);
        const uint32_t skew = (uint32_t)(a & 3), last = (skew + n - 1) >> 2;
        for (uint32_t j = (uint32_t)ln; j < nd + 2; j += 64) {
            const uint64_t lo = j <= last ? g32[j] : 0u, hi = j + 1 <= last ? g32[j + 1] : 0u;
            s_pay[wave][j] = (uint32_t)((lo | (hi << 32)) >> (skew * 8));
        }
    }
    def_wave_sync();
    LfqDefDevIo io;
    io.pay = (LfqDefLdsU32 *)s_pay[wave];
    io.slot = (uint32_t *)(A.slots + lfq_def_slot_off(off, b));
    io.slot_dwords = (5 + n + 3) >> 2;
    io.ln = ln;
    /* CRC-32: a slice of whole dwords per lane, then each slice's CRC times x^(8 * bytes behind it), summed over the lanes */
    {
        const uint32_t each = lfq_crc_slice_bytes(n);
        const uint32_t a = min((uint32_t)ln * each, n), e = min(a + each, n);
        uint32_t crc = 0xffffffffu, i = a;
        for (; i + 4 <= e; i += 4) {
            uint32_t w = io.pay[i >> 2];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                crc = s_crc[(crc ^ w) & 0xffu] ^ (crc >> 8);
                w >>= 8;
            }
        }
        for (; i < e; i++) {
            crc = s_crc[(crc ^ io.ld8(i)) & 0xffu] ^ (crc >> 8);
        }
        crc = e > a ? ~crc : 0u;
        crc = lfq_crc_mul(lfq_crc_x8n(n - e), crc);
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            crc ^= (uint32_t)__shfl_xor((int)crc, m, 64);
        }
        if (ln == 0) {
            A.crc[b] = crc;
        }
    }
    const LfqDefResult R = lfq_deflate(&s_st[wave], n, io);
    if (ln == 0) {
        A.res[b] = R;
    }
}

/* One aligned dword of the final bytes per thread.  Byte o of block b: the 18 header bytes (the last two: the block's size - 1), the
 * stream from its slot, CRC-32 and ISIZE. */
__device__ __forceinline__ uint32_t def_block_byte(const LfqDefArgs &A, int64_t b, int64_t o)
{
    const int64_t size = A.comp_off[b + 1] - A.comp_off[b];
    if (o < LFQ_BGZF_HEAD) {
        const uint64_t h0 = 0x00000000'04088b1full, h1 = 0x00024342'0006ff00ull;   /* 1f 8b 08 04 00 00 00 00 | 00 ff 06 00 42 43 02 00 */
        return o < 8 ? (uint32_t)(h0 >> (8 * o)) & 0xffu : o < 16 ? (uint32_t)(h1 >> (8 * (o - 8))) & 0xffu
                                                                  : (uint32_t)((size - 1) >> (8 * (o - 16))) & 0xffu;
    }
    const int64_t tail = size - LFQ_BGZF_TAIL;
    if (o < tail) {
        return A.slots[lfq_def_slot_off(A.data_off[b], b) + (o - LFQ_BGZF_HEAD)];
    }
    const uint32_t v = o < tail + 4 ? A.crc[b] : (uint32_t)(A.data_off[b + 1] - A.data_off[b]);
    return (v >> (8 * ((o - tail) & 3))) & 0xffu;
}

__global__ __launch_bounds__(LFQ_BGZF_PACK_THREADS) void lfq_bgzf_pack_kernel(LfqDefArgs A)
{
    const int64_t g = ((int64_t)blockIdx.x * LFQ_BGZF_PACK_THREADS + threadIdx.x) * 4, total = A.comp_off[A.n_blocks];
    if (g >= total) {
        return;
    }
    int64_t lo = 0, hi = A.n_blocks - 1;        /* the block of byte g: the last one that starts at or in front of it */
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (A.comp_off[mid] <= g) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    int64_t b = lo;
    const int64_t o = g - A.comp_off[b], s_end = A.comp_off[b + 1] - A.comp_off[b] - LFQ_BGZF_TAIL;
    uint32_t v = 0;
    if (o >= LFQ_BGZF_HEAD && o + 4 <= s_end) {
        /* four bytes of the stream: from the two aligned dwords of the slot around them */
        const int64_t at = o - LFQ_BGZF_HEAD;
        const uint32_t *s32 = (const uint32_t *)(A.slots + lfq_def_slot_off(A.data_off[b], b)) + (at >> 2);
        const uint32_t sh = (uint32_t)(at & 3) * 8;
        v = sh ? (s32[0] >> sh) | (s32[1] << (32 - sh)) : s32[0];
    } else {
        for (int k = 0; k < 4; k++) {
            int64_t p = g + k;
            if (p >= total) {
                break;
            }
            while (p >= A.comp_off[b + 1]) {    /* (blocks are 27 bytes at least: one trip at most) */
                b++;
            }
            v |= def_block_byte(A, b, p - A.comp_off[b]) << (8 * k);
        }
    }
    A.comp[g >> 2] = v;
}

/* ---- host side ------------------------------------------------------------------------------------------------------------------- */
static const uint8_t lfq_bgzf_eof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0,
                                         0, 0, 0, 0, 0, 0, 0, 0};

struct LfqBgzfDefState {
    uint8_t *d_in = nullptr;            /* the input, when it is not on the device already (grow-only, as all of these) */
    int64_t d_in_bytes = 0;
    uint8_t *d_buf = nullptr;           /* data_off | comp_off | results | CRCs | slots */
    int64_t d_bytes = 0;
    uint8_t *d_comp = nullptr;
    int64_t d_comp_bytes = 0;
    uint8_t *h_stage = nullptr;         /* pinned staging of input that comes in pageable memory */
    int64_t h_stage_bytes = 0;
    uint8_t *h_comp = nullptr;          /* the blocks on the host, pinned */
    int64_t h_comp_bytes = 0;
    std::vector<int64_t> data_off, comp_off;
    std::vector<uint8_t> btype;
    uint8_t none[32] = {};
    lfq_bgzf_deflated result = {};
    lfq_bgzf_deflate_times times = {};
    LfqEvPair up_t = {}, kern_t = {}, down_t = {};
};

static LfqBgzfDefState *bgzf_def_state(lfq_ctx *c)
{
    if (!c->bgzf_def) {
        c->bgzf_def = new LfqBgzfDefState();
    }
    return c->bgzf_def;
}

void lfq_bgzf_deflate_release(lfq_ctx *c)
{
    if (LfqBgzfDefState *S = c->bgzf_def) {
        if (S->d_in) (void)hipFree(S->d_in);
        if (S->d_buf) (void)hipFree(S->d_buf);
        if (S->d_comp) (void)hipFree(S->d_comp);
        free_pinned(&S->h_stage, &S->h_stage_bytes);
        free_pinned(&S->h_comp, &S->h_comp_bytes);
        for (LfqEvPair *t : {&S->up_t, &S->kern_t, &S->down_t}) {
            t->destroy();
        }
        delete S;
        c->bgzf_def = nullptr;
    }
}

static int bgzf_def_add_ms(const LfqEvPair &t, double *acc)
{
    double ms = 0.0;
    LFQ_TRY(t.ms(&ms));
    *acc += ms;
    return LFQ_OK;
}

extern "C" int lfq_bgzf_deflate(lfq_ctx *c, const uint8_t *data, int64_t n_bytes, const int64_t *cuts, int64_t n_cuts, unsigned flags,
                                const lfq_bgzf_deflated **out)
{
    if (out) *out = nullptr;
    if (!c || !out || n_bytes < 0 || (n_bytes > 0 && !data) || (flags & ~(unsigned)LFQ_BGZF_PUT_EOF) || n_cuts < 0
        || (n_cuts > 0 && !cuts)) {
        return LFQ_ERR_INVALID;
    }
    std::vector<int64_t> data_off(1, 0);
    if (cuts) {
        for (int64_t i = 0; i < n_cuts; i++) {
            if (cuts[i] <= data_off.back() || cuts[i] >= n_bytes) {
                return LFQ_ERR_INVALID;
            }
            data_off.push_back(cuts[i]);
        }
    } else {
        for (int64_t p = LFQ_DEF_MAX_IN; p < n_bytes; p += LFQ_DEF_MAX_IN) {
            data_off.push_back(p);
        }
    }
    if (n_bytes > 0) {
        data_off.push_back(n_bytes);
    }
    const int64_t nb = (int64_t)data_off.size() - 1;
    for (int64_t b = 0; b < nb; b++) {
        if (data_off[(size_t)b + 1] - data_off[(size_t)b] > LFQ_DEF_MAX_IN) {
            return LFQ_ERR_INVALID;
        }
    }
    const bool eof = (flags & LFQ_BGZF_PUT_EOF) != 0;
    LfqBgzfDefState *S = bgzf_def_state(c);
    S->data_off.swap(data_off);
    S->comp_off.assign((size_t)nb + 1, 0);
    S->btype.assign((size_t)std::max<int64_t>(nb, 1), 0);
    S->times = {};
    S->times.n_blocks = nb;
    S->times.n_in_bytes = n_bytes;
    lfq_bgzf_deflated &R = S->result;
    R.n_blocks = nb;
    R.data_off = S->data_off.data();
    R.comp_off = S->comp_off.data();
    R.btype = S->btype.data();
    if (nb == 0) {
        memcpy(S->none, lfq_bgzf_eof, sizeof(lfq_bgzf_eof));
        R.comp = S->none;
        R.n_bytes = S->times.n_out_bytes = eof ? (int64_t)sizeof(lfq_bgzf_eof) : 0;
        *out = &R;
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    /* the payload: where it lies on the device already, or one copy down */
    const uint8_t *d_data = lfq_bgzf_resident_bytes(c, data, n_bytes);
    if (!d_data) {
        d_data = lfq_bam_framed_resident(c, data, n_bytes);
    }
    const int64_t o_coff = lfq_al((nb + 1) * 8), o_res = o_coff + lfq_al((nb + 1) * 8), o_crc = o_res + lfq_al(nb * 8),
                  o_slots = o_crc + lfq_al(nb * 4), total = o_slots + lfq_al(lfq_def_slot_off(n_bytes, nb) + 16);
    LFQ_TRY(grow(&S->d_buf, &S->d_bytes, total));
    LfqPin<int64_t> offs(c, (size_t)nb + 1);
    LFQ_PIN_OK(offs);
    memcpy(offs.data(), S->data_off.data(), (size_t)(nb + 1) * 8);
    LFQ_TRY(S->up_t.begin(st));
    if (d_data) {
        S->times.n_from_device = 1;
    } else {
        LFQ_TRY(grow(&S->d_in, &S->d_in_bytes, lfq_al(n_bytes + 16)));
        const uint8_t *src = data;
        if (!lfq_is_pinned(data)) {
            if (n_bytes > S->h_stage_bytes) {
                LFQ_TRY(grow_pinned(&S->h_stage, &S->h_stage_bytes, std::max<int64_t>(n_bytes + n_bytes / 4, 1 << 16)));
            }
            memcpy(S->h_stage, data, (size_t)n_bytes);
            src = S->h_stage;
        }
        LFQ_TRY_HIP(hipMemcpyAsync(S->d_in, src, (size_t)n_bytes, hipMemcpyHostToDevice, st));
        d_data = S->d_in;
    }
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf, offs.data(), (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, st));
    LFQ_TRY(S->up_t.end(st));
    LfqDefArgs A;
    memset(&A, 0, sizeof(A));
    A.data = d_data;
    A.data_off = (const int64_t *)S->d_buf;
    A.comp_off = (const int64_t *)(S->d_buf + o_coff);
    A.res = (LfqDefResult *)(S->d_buf + o_res);
    A.crc = (uint32_t *)(S->d_buf + o_crc);
    A.slots = S->d_buf + o_slots;
    A.n_blocks = nb;
    LFQ_TRY(S->kern_t.begin(st));
    hipLaunchKernelGGL(lfq_bgzf_deflate_kernel, dim3((unsigned)((nb + LFQ_BGZF_DEF_BLOCKS_PER_WG - 1) / LFQ_BGZF_DEF_BLOCKS_PER_WG)),
                       dim3(64 * LFQ_BGZF_DEF_BLOCKS_PER_WG), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    S->times.n_launches = 1;
    LfqPin<LfqDefResult> res(c, (size_t)nb);
    LFQ_PIN_OK(res);
    LFQ_TRY(S->down_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(res.data(), A.res, (size_t)nb * sizeof(LfqDefResult), hipMemcpyDeviceToHost, st));
    LFQ_TRY(S->down_t.end(st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bgzf_def_add_ms(S->up_t, &S->times.upload_ms));
    LFQ_TRY(bgzf_def_add_ms(S->kern_t, &S->times.kernels_ms));
    LFQ_TRY(bgzf_def_add_ms(S->down_t, &S->times.download_ms));
    for (int64_t b = 0; b < nb; b++) {
        const int64_t n = S->data_off[(size_t)b + 1] - S->data_off[(size_t)b];
        if (res[(size_t)b].btype > LFQ_DEF_DYNAMIC || res[(size_t)b].n_bytes > 5 + n || res[(size_t)b].n_bytes == 0) {
            return LFQ_ERR_HIP;                 /* the kernel's two passes disagree, or it did not run */
        }
        S->btype[(size_t)b] = (uint8_t)res[(size_t)b].btype;
        S->comp_off[(size_t)b + 1] = S->comp_off[(size_t)b] + LFQ_BGZF_HEAD + res[(size_t)b].n_bytes + LFQ_BGZF_TAIL;
    }
    const int64_t n_comp = S->comp_off[(size_t)nb], n_out = n_comp + (eof ? (int64_t)sizeof(lfq_bgzf_eof) : 0);
    LFQ_TRY(grow(&S->d_comp, &S->d_comp_bytes, lfq_al(n_comp + 16)));
    if (n_out + 16 > S->h_comp_bytes) {
        LFQ_TRY(grow_pinned(&S->h_comp, &S->h_comp_bytes, std::max<int64_t>(n_out + n_out / 4 + 16, 1 << 16)));
    }
    A.comp = (uint32_t *)S->d_comp;
    memcpy(offs.data(), S->comp_off.data(), (size_t)(nb + 1) * 8);
    LFQ_TRY(S->up_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(S->d_buf + o_coff, offs.data(), (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, st));
    LFQ_TRY(S->up_t.end(st));
    LFQ_TRY(S->kern_t.begin(st));
    const int64_t n_dwords = (n_comp + 3) / 4;
    hipLaunchKernelGGL(lfq_bgzf_pack_kernel, dim3((unsigned)((n_dwords + LFQ_BGZF_PACK_THREADS - 1) / LFQ_BGZF_PACK_THREADS)),
                       dim3(LFQ_BGZF_PACK_THREADS), 0, st, A);
    LFQ_TRY_HIP(hipGetLastError());
    LFQ_TRY(S->kern_t.end(st));
    S->times.n_launches = 2;
    LFQ_TRY(S->down_t.begin(st));
    LFQ_TRY_HIP(hipMemcpyAsync(S->h_comp, S->d_comp, (size_t)n_comp, hipMemcpyDeviceToHost, st));
    LFQ_TRY(S->down_t.end(st));
    LFQ_TRY_HIP(hipStreamSynchronize(st));
    LFQ_TRY(bgzf_def_add_ms(S->up_t, &S->times.upload_ms));
    LFQ_TRY(bgzf_def_add_ms(S->kern_t, &S->times.kernels_ms));
    LFQ_TRY(bgzf_def_add_ms(S->down_t, &S->times.download_ms));
    if (eof) {
        memcpy(S->h_comp + n_comp, lfq_bgzf_eof, sizeof(lfq_bgzf_eof));
    }
    R.comp = S->h_comp;
    R.n_bytes = S->times.n_out_bytes = n_out;
    *out = &R;
    return LFQ_OK;
}

extern "C" int lfq_last_bgzf_deflate_times(lfq_ctx *c, lfq_bgzf_deflate_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = bgzf_def_state(c)->times;
    return LFQ_OK;
}
