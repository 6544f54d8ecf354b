/*
 * lfq_fasta.hip -- `lofreq faidx` and the contig of a FASTA on the device (include/lofreq_amd.h: lfq_fasta_*), over lfq_fasta.h.
 *
 *   scan     three launches over the resident file bytes, a lane per chunk of 16 aligned bytes (one dwordx4 load):
 *              tiles   the chunk's graph bytes, line-starting newlines and headers from its masks; a workgroup scan gives the
 *                      graph rank of every chunk inside its tile (32 bit) and the tile's three sums
 *              sums    one wavefront scans the tiles' sums (64 bit), LFQ_FA_SCAN_LANES tiles a round
 *              emit    the masks again; the start of every line and the line number of every header go to their slots
 *            No launch waits for another workgroup of itself: the hand-over between the three is the launch boundary.
 *   lines    a lane per line.  chain: the first line of every sequence that is not full, an atomic min per sequence; legal: the
 *            first offending line of the file, an atomic min over (line, why).  Both find a line's sequence by binary search in the
 *            header list the emit launch left (a max-scan over the lines would be a second three-launch scan for the same answer).
 *   entries  a lane per header: lfq_fa_name_cut, offset, line_len, and length / line_blen as differences of graph ranks.
 *   fetch    output-major, a lane per 16 aligned bases, one dwordx4 store.
 *              regular   base p from offset + p / blen * llen + p % blen: aligned dwords, funnel-shifted; bytes at a line's seam.
 *                        Only after lfq_fasta_prove_kernel, a lane per line of the span, has found every line but the last to be
 *                        blen graph bytes and '\n' (llen == blen + 1: a "\r\n" file takes the general path, counts cannot tell
 *                        where in a line its '\r' stands).
 *              general   the p-th graph byte at or behind offset by rank: binary search in the tile bases, then in the tile's
 *                        chunk ranks, then the chunk's mask, then a walk over the masks for the lane's other 15.
 *            Every entry, built or parsed, is checked on the host first: offset inside the file, `length` graph bytes behind it.
 */
#include "lfq_ctx.h"
#include "lfq_fasta.h"

/* the resident file as the kernels see it.  bytes[] is padded with zeros to a multiple of 16 plus 16: a chunk load and the aligned
 * dword around the file's last byte stay inside the allocation, and a zero is in no class */
struct LfqFaView {
    const uint8_t *bytes;
    int64_t n, n_chunks, n_tiles, n_lines, n_hdr;
    uint32_t *crank;                    /* [n_chunks] graph bytes of the tile in front of the chunk */
    int64_t *tile_g, *tile_nl, *tile_hd; /* [n_tiles + 1] sums, then exclusive bases; [n_tiles]: the totals */
    int64_t *lstart;                    /* [n_lines + 1] */
    int64_t *hline;                     /* [n_hdr] the line of every header */
};

struct LfqFaChunk {
    uint32_t graph, starts, hdr;        /* masks: graph bytes; newlines that start a line; first bytes of header lines */
};

__device__ __forceinline__ LfqFaChunk fa_chunk(const LfqFaView &V, int64_t c)
{
    const uint4 w = *reinterpret_cast<const uint4 *>(V.bytes + c * LFQ_FA_CHUNK);
    const LfqFaMasks m = lfq_fa_chunk_masks(w.x, w.y, w.z, w.w);
    const uint32_t prev_nl = c == 0 ? 1u : (uint32_t)(V.bytes[c * LFQ_FA_CHUNK - 1] == '\n');   /* the file's start starts a line */
    LfqFaChunk k;
    k.graph = m.graph;
    k.starts = lfq_fa_line_starts(m.nl, c, V.n);
    k.hdr = ((m.nl << 1) | prev_nl) & m.gt & 0xffffu;
    return k;
}

#define FA_PACK(g, nl, hd) ((uint64_t)(g) | ((uint64_t)(nl) << 20) | ((uint64_t)(hd) << 40))
#define FA_FIELD(x, i) ((uint32_t)((x) >> (20 * (i))) & 0xfffffu)

__device__ __forceinline__ uint64_t fa_wave_incl(uint64_t x)
{
    const int lane = (int)(threadIdx.x & 63);
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)x, d, 64), hi = __shfl_up((uint32_t)(x >> 32), d, 64);
        if (lane >= d) {
            x += ((uint64_t)hi << 32) | lo;
        }
    }
    return x;
}

/* exclusive scan of v over the workgroup (chunk order); *total: the workgroup's sum.  Once per kernel */
__device__ __forceinline__ uint64_t fa_block_exscan(uint64_t v, uint64_t *s_w, uint64_t *total)
{
    const int wv = (int)(threadIdx.x >> 6);
    const uint64_t x = fa_wave_incl(v);
    if ((threadIdx.x & 63) == 63) {
        s_w[wv] = x;
    }
    __syncthreads();
    uint64_t base = 0, all = 0;
    for (int i = 0; i < LFQ_FA_THREADS / 64; i++) {
        base += i < wv ? s_w[i] : 0;
        all += s_w[i];
    }
    *total = all;
    return base + x - v;
}

__global__ __launch_bounds__(LFQ_FA_THREADS) void lfq_fasta_tiles_kernel(LfqFaView V)
{
    __shared__ uint64_t s_w[LFQ_FA_THREADS / 64];
    const int64_t c = (int64_t)blockIdx.x * LFQ_FA_THREADS + threadIdx.x;
    uint64_t v = 0;
    if (c < V.n_chunks) {
        const LfqFaChunk k = fa_chunk(V, c);
        v = FA_PACK(__popc(k.graph), __popc(k.starts), __popc(k.hdr));
    }
    uint64_t total;
    const uint64_t ex = fa_block_exscan(v, s_w, &total);
    if (c < V.n_chunks) {
        V.crank[c] = FA_FIELD(ex, 0);
    }
    if (threadIdx.x == 0) {
        V.tile_g[blockIdx.x] = FA_FIELD(total, 0);
        V.tile_nl[blockIdx.x] = FA_FIELD(total, 1);
        V.tile_hd[blockIdx.x] = FA_FIELD(total, 2);
    }
}

__device__ __forceinline__ int64_t fa_wave_incl_i64(int64_t x) { return (int64_t)fa_wave_incl((uint64_t)x); }

/* one wavefront: the three sums per tile -> exclusive bases, in place; slot n_tiles gets the totals */
__global__ __launch_bounds__(LFQ_FA_SCAN_LANES) void lfq_fasta_sums_kernel(LfqFaView V)
{
    int64_t base[3] = {0, 0, 0};
    int64_t *const arr[3] = {V.tile_g, V.tile_nl, V.tile_hd};
    for (int64_t t0 = 0; t0 < V.n_tiles; t0 += LFQ_FA_SCAN_LANES) {
        const int64_t t = t0 + threadIdx.x;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const int64_t in = t < V.n_tiles ? arr[a][t] : 0;
            const int64_t inc = fa_wave_incl_i64(in);
            if (t < V.n_tiles) {
                arr[a][t] = base[a] + inc - in;
            }
            const uint32_t lo = __shfl((uint32_t)inc, 63, 64), hi = __shfl((uint32_t)((uint64_t)inc >> 32), 63, 64);
            base[a] += (int64_t)(((uint64_t)hi << 32) | lo);
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            arr[a][V.n_tiles] = base[a];
        }
    }
}

__global__ __launch_bounds__(LFQ_FA_THREADS) void lfq_fasta_emit_kernel(LfqFaView V)
{
    __shared__ uint64_t s_w[LFQ_FA_THREADS / 64];
    const int64_t c = (int64_t)blockIdx.x * LFQ_FA_THREADS + threadIdx.x;
    LfqFaChunk k = {0, 0, 0};
    if (c < V.n_chunks) {
        k = fa_chunk(V, c);
    }
    uint64_t total;
    const uint64_t ex = fa_block_exscan(FA_PACK(0, __popc(k.starts), __popc(k.hdr)), s_w, &total);
    const int64_t nl0 = V.tile_nl[blockIdx.x] + FA_FIELD(ex, 1);       /* line-starting newlines in front of the chunk */
    int64_t hd = V.tile_hd[blockIdx.x] + FA_FIELD(ex, 2);
    int64_t nl = nl0;
    for (uint32_t m = k.starts; m; m &= m - 1) {
        const int i = __ffs((int)m) - 1;
        V.lstart[1 + nl++] = c * LFQ_FA_CHUNK + i + 1;                  /* (1 + nl <= n_lines - 1: by the count of the same mask) */
    }
    for (uint32_t m = k.hdr; m; m &= m - 1) {
        const int i = __ffs((int)m) - 1;
        V.hline[hd++] = nl0 + __popc(k.starts & ((1u << i) - 1u));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        V.lstart[0] = 0;
        V.lstart[V.n_lines] = V.bytes[V.n - 1] == '\n' ? V.n : V.n + 1;
    }
}

/* the graph bytes in front of byte x, 0 <= x <= n */
__device__ __forceinline__ int64_t fa_rank(const LfqFaView &V, int64_t x)
{
    if (x >= V.n) {
        return V.tile_g[V.n_tiles];
    }
    const int64_t c = x / LFQ_FA_CHUNK;
    const uint4 w = *reinterpret_cast<const uint4 *>(V.bytes + c * LFQ_FA_CHUNK);
    const uint32_t g = lfq_fa_chunk_masks(w.x, w.y, w.z, w.w).graph;
    return V.tile_g[c / LFQ_FA_THREADS] + V.crank[c] + __popc(g & ((1u << (x % LFQ_FA_CHUNK)) - 1u));
}

/* the sequence of line k: the last header at or in front of it, -1: none */
__device__ __forceinline__ int64_t fa_seq_of(const LfqFaView &V, int64_t k)
{
    int64_t lo = 0, hi = V.n_hdr;       /* -> the number of headers with hline <= k */
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (V.hline[mid] <= k) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo - 1;
}

#define FA_NONE 0xffffffffffffffffull

__global__ __launch_bounds__(256) void lfq_fasta_chain_kernel(LfqFaView V, unsigned long long *__restrict__ seq_m)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= V.n_lines) {
        return;
    }
    const int64_t s = V.lstart[k];
    if (V.bytes[s] == '>') {
        return;
    }
    const int64_t h = fa_seq_of(V, k);
    if (h < 0) {
        return;
    }
    const int64_t f = V.hline[h] + 1;
    if (!lfq_fa_line_full(V.lstart[k + 1] - s, V.lstart[f + 1] - V.lstart[f])) {
        atomicMin(&seq_m[h], (unsigned long long)k);
    }
}

__global__ __launch_bounds__(256) void lfq_fasta_legal_kernel(LfqFaView V, const unsigned long long *__restrict__ seq_m,
                                                              unsigned long long *__restrict__ bad)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= V.n_lines) {
        return;
    }
    const int64_t s = V.lstart[k], bytes = V.lstart[k + 1] - s;
    const int b0 = V.bytes[s];
    if (b0 == '>') {
        return;
    }
    const int64_t h = fa_seq_of(V, k);
    int64_t m = -1, fb = 0;
    if (h >= 0) {
        const int64_t f = V.hline[h] + 1;
        fb = V.lstart[f + 1] - V.lstart[f];
        m = seq_m[h] == FA_NONE ? INT64_MAX : (int64_t)seq_m[h];
    }
    const int b1 = s + 1 < V.n ? (int)V.bytes[s + 1] : -1;
    const int off = lfq_fa_line_offence(k, m, bytes, fb, lfq_fa_line_skippable(bytes, b0, b1));
    if (off != LFQ_FA_OK) {
        atomicMin(bad, ((unsigned long long)k << 2) | (unsigned long long)off);
    }
}

__global__ __launch_bounds__(256) void lfq_fasta_entries_kernel(LfqFaView V, const unsigned long long *__restrict__ seq_m,
                                                                LfqFaRaw *__restrict__ raw)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= V.n_hdr) {
        return;
    }
    const int64_t hl = V.hline[h], f = hl + 1, last = (h + 1 < V.n_hdr ? V.hline[h + 1] : V.n_lines) - 1;
    LfqFaRaw r;
    r.offset = V.lstart[f];
    r.length = 0;
    r.line_blen = r.line_len = 0;
    const int64_t hdr_end = r.offset <= V.n ? r.offset - 1 : V.n;       /* the header's '\n', or the file's end */
    int64_t nb, nl;
    lfq_fa_name_cut(V.bytes, V.lstart[hl] + 1, hdr_end, &nb, &nl);
    r.name_beg = nb;
    r.name_len = (int32_t)nl;
    r.valid = f <= last && V.lstart[f + 1] - V.lstart[f] != 1;
    if (r.valid) {
        const int64_t m = seq_m[h] == FA_NONE ? last : min((int64_t)seq_m[h], last), r0 = fa_rank(V, r.offset);
        r.length = fa_rank(V, min(V.lstart[m + 1], V.n)) - r0;
        r.line_len = (int32_t)(V.lstart[f + 1] - V.lstart[f]);
        r.line_blen = (int32_t)(fa_rank(V, min(V.lstart[f + 1], V.n)) - r0);
    }
    raw[h] = r;
}

/* the names, one behind the other: a lane per header, a byte at a time (a file has few headers and their names are short) */
__global__ __launch_bounds__(256) void lfq_fasta_names_kernel(LfqFaView V, const LfqFaRaw *__restrict__ raw,
                                                              const int64_t *__restrict__ name_off, uint8_t *__restrict__ out)
{
    const int64_t h = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (h >= V.n_hdr) {
        return;
    }
    const int64_t beg = raw[h].name_beg, n = name_off[h + 1] - name_off[h];
    for (int64_t i = 0; i < n; i++) {
        out[name_off[h] + i] = V.bytes[beg + i];
    }
}

struct LfqFaFetch {
    int64_t offset, length, blen, llen;
    int64_t r0;                         /* graph bytes in front of offset */
    uint8_t *out;                       /* 16-byte aligned */
};

/* a lane per line of the span: bit 0 of *flag when the span is not regular.  The host has checked that the span's last byte, as the
 * formula places it, lies inside the file */
__global__ __launch_bounds__(256) void lfq_fasta_prove_kernel(LfqFaView V, LfqFaFetch F, int64_t n_span, unsigned int *__restrict__ flag)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_span) {
        return;
    }
    const int64_t s = F.offset + k * F.llen;
    int64_t lo = 0, hi = V.n_lines;     /* -> the first line that starts at or behind s */
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (V.lstart[mid] < s) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    bool ok = lo < V.n_lines && V.lstart[lo] == s;
    if (ok && k + 1 < n_span) {
        const int64_t e = V.lstart[lo + 1];
        ok = e - s == F.llen && fa_rank(V, min(e, V.n)) - fa_rank(V, s) == F.blen;
    } else if (ok) {
        const int64_t rem = F.length - k * F.blen;
        ok = s + rem <= V.n && fa_rank(V, s + rem) - fa_rank(V, s) == rem;
    }
    if (!ok) {
        atomicOr(flag, 1u);
    }
}

__device__ __forceinline__ void fa_store16(const LfqFaFetch &F, int64_t p0, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3)
{
    if (p0 + 16 <= F.length) {
        *reinterpret_cast<uint4 *>(F.out + p0) = make_uint4(o0, o1, o2, o3);
        return;
    }
    for (int j = 0; p0 + j < F.length; j++) {           /* the contig's tail: no store behind its last base */
        const uint32_t w = j < 4 ? o0 : j < 8 ? o1 : j < 12 ? o2 : o3;
        F.out[p0 + j] = (uint8_t)(w >> ((j & 3) * 8));
    }
}

__global__ __launch_bounds__(256) void lfq_fasta_fetch_regular_kernel(LfqFaView V, LfqFaFetch F)
{
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= F.length) {
        return;
    }
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const int64_t p = p0 + 4 * d, q = p / F.blen, r = p - q * F.blen;
        uint32_t v = 0;
        if (p + 4 <= F.length && r + 4 <= F.blen) {     /* four bases of one line: two aligned dwords, funnel-shifted */
            const int64_t src = F.offset + q * F.llen + r, a = src & ~(int64_t)3;
            const uint32_t sh = (uint32_t)(src & 3) * 8u;
            v = *reinterpret_cast<const uint32_t *>(V.bytes + a);
            if (sh) {
                v = __funnelshift_r(v, *reinterpret_cast<const uint32_t *>(V.bytes + a + 4), sh);
            }
        } else {                                        /* a line's seam or the contig's end */
            for (int b = 0; b < 4 && p + b < F.length; b++) {
                v |= (uint32_t)V.bytes[lfq_fa_regular_src(F.offset, p + b, F.blen, F.llen)] << (8 * b);
            }
        }
        o[d] = v;
    }
    fa_store16(F, p0, o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void lfq_fasta_fetch_general_kernel(LfqFaView V, LfqFaFetch F)
{
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= F.length) {
        return;
    }
    const int64_t R = F.r0 + p0;                        /* the rank of the lane's first base: R < the file's graph bytes (host) */
    int64_t lo = 0, hi = V.n_tiles;                     /* -> the last tile whose base is <= R */
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (V.tile_g[mid] <= R) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    const uint32_t rt = (uint32_t)(R - V.tile_g[lo]);
    int64_t c = lo * LFQ_FA_THREADS, ce = min(c + LFQ_FA_THREADS, V.n_chunks);
    while (ce - c > 1) {                                /* -> the last chunk of the tile whose rank is <= rt */
        const int64_t mid = c + ((ce - c) >> 1);
        if (V.crank[mid] <= rt) {
            c = mid;
        } else {
            ce = mid;
        }
    }
    uint4 w = *reinterpret_cast<const uint4 *>(V.bytes + c * LFQ_FA_CHUNK);
    uint32_t mask = lfq_fa_chunk_masks(w.x, w.y, w.z, w.w).graph;
    for (uint32_t skip = rt - V.crank[c]; skip && mask; skip--) {
        mask &= mask - 1;
    }
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (p0 + j < F.length) {
            while (!mask && c + 1 < V.n_chunks) {       /* ends: the host has counted `length` graph bytes behind offset */
                c++;
                w = *reinterpret_cast<const uint4 *>(V.bytes + c * LFQ_FA_CHUNK);
                mask = lfq_fa_chunk_masks(w.x, w.y, w.z, w.w).graph;
            }
            if (mask) {
                const int i = __ffs((int)mask) - 1;
                mask &= mask - 1;
                const uint32_t word = i < 4 ? w.x : i < 8 ? w.y : i < 12 ? w.z : w.w;
                o[j >> 2] |= ((word >> ((i & 3) * 8)) & 0xffu) << ((j & 3) * 8);
            }
        }
    }
    fa_store16(F, p0, o[0], o[1], o[2], o[3]);
}

/* ---- host ---------------------------------------------------------------------------------------------------------------------------- */
struct lfq_fasta {
    lfq_ctx *c;
    LfqFaView V;
    uint8_t *d_blob;                    /* bytes | crank | tile sums */
    uint8_t *d_lines;                   /* lstart | hline */
    std::vector<int64_t> tile_g;        /* the tile bases on the host: where a parsed offset stands by rank */
    int64_t total_graph;
    uint8_t *d_seq, *h_seq;             /* the contig handed out last */
    int64_t d_seq_cap, h_seq_cap;
    lfq_fasta_contig contig;
};

struct LfqFastaState {
    lfq_fasta_times times;
    LfqEvPair scan_t, lines_t, fetch_t;
    bool scan_on, lines_on, fetch_on;
    lfq_fasta *live;                    /* the file whose contig is the context's live fetch result */
};

static LfqFastaState *fa_state(lfq_ctx *c)
{
    if (!c->fasta) {
        c->fasta = new LfqFastaState();
        memset(&c->fasta->times, 0, sizeof(c->fasta->times));
        memset(c->fasta->scan_t.ev, 0, sizeof(c->fasta->scan_t.ev));
        memset(c->fasta->lines_t.ev, 0, sizeof(c->fasta->lines_t.ev));
        memset(c->fasta->fetch_t.ev, 0, sizeof(c->fasta->fetch_t.ev));
        c->fasta->scan_on = c->fasta->lines_on = c->fasta->fetch_on = false;
        c->fasta->live = nullptr;
    }
    return c->fasta;
}

void lfq_fasta_release(lfq_ctx *c)
{
    if (LfqFastaState *S = c->fasta) {
        for (LfqEvPair *t : {&S->scan_t, &S->lines_t, &S->fetch_t}) {
            t->destroy();
        }
        delete S;
        c->fasta = nullptr;
    }
}

const uint8_t *lfq_fasta_resident(lfq_ctx *c, const uint8_t *p, int64_t bytes)
{
    LfqFastaState *S = c->fasta;
    if (!S || !S->live || !p || bytes <= 0) {
        return nullptr;
    }
    const lfq_fasta_contig &g = S->live->contig;
    if (!g.seq || p < g.seq || p + bytes > g.seq + g.len) {
        return nullptr;
    }
    S->times.n_handovers += 1;
    return S->live->d_seq + (p - g.seq);
}

static inline unsigned fa_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

static bool fa_launched() { return hipGetLastError() == hipSuccess; }

extern "C" {

void lfq_fasta_close(lfq_fasta *fa)
{
    if (!fa) {
        return;
    }
    (void)hipSetDevice(fa->c->device);
    if (fa->c->fasta && fa->c->fasta->live == fa) {
        fa->c->fasta->live = nullptr;
    }
    if (fa->d_blob) (void)hipFree(fa->d_blob);
    if (fa->d_lines) (void)hipFree(fa->d_lines);
    if (fa->d_seq) (void)hipFree(fa->d_seq);
    free_pinned(&fa->h_seq, &fa->h_seq_cap);
    delete fa;
}

int lfq_fasta_open(lfq_ctx *c, const uint8_t *bytes, int64_t n, lfq_fasta **out)
{
    if (!c || !out || n < 0 || (n > 0 && !bytes)) {
        return LFQ_ERR_INVALID;
    }
    *out = nullptr;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LfqFastaState *S = fa_state(c);
    memset(&S->times, 0, sizeof(S->times));
    S->scan_on = S->lines_on = S->fetch_on = false;
    lfq_fasta *fa = new lfq_fasta();
    fa->c = c;
    memset(&fa->V, 0, sizeof(fa->V));
    fa->d_blob = fa->d_lines = fa->d_seq = fa->h_seq = nullptr;
    fa->d_seq_cap = fa->h_seq_cap = 0;
    fa->total_graph = 0;
    memset(&fa->contig, 0, sizeof(fa->contig));
    LfqFaView &V = fa->V;
    V.n = n;
    V.n_chunks = (n + LFQ_FA_CHUNK - 1) / LFQ_FA_CHUNK;
    V.n_tiles = (V.n_chunks + LFQ_FA_THREADS - 1) / LFQ_FA_THREADS;
    S->times.n_bytes = n;
    if (n == 0) {
        *out = fa;
        return LFQ_OK;
    }
    hipStream_t st = c->stream;
    const int64_t padded = V.n_chunks * LFQ_FA_CHUNK + 16, o_rank = lfq_al(padded), o_tg = o_rank + lfq_al(V.n_chunks * 4),
                  o_tn = o_tg + lfq_al((V.n_tiles + 1) * 8), o_th = o_tn + lfq_al((V.n_tiles + 1) * 8),
                  total = o_th + lfq_al((V.n_tiles + 1) * 8);
    int rc = LFQ_OK;
    auto fail = [&](int why) {
        lfq_fasta_close(fa);
        return why;
    };
    if (hipMalloc((void **)&fa->d_blob, (size_t)total) != hipSuccess) {
        fa->d_blob = nullptr;
        return fail(LFQ_ERR_NOMEM);
    }
    uint8_t *d = fa->d_blob;
    V.bytes = d;
    V.crank = (uint32_t *)(d + o_rank);
    V.tile_g = (int64_t *)(d + o_tg);
    V.tile_nl = (int64_t *)(d + o_tn);
    V.tile_hd = (int64_t *)(d + o_th);
    /* the file: from the context's live inflate result when it lies there (a bgzip-compressed FASTA), else across the link */
    const double t0 = lfq_now_ms();
    const uint8_t *res = lfq_bgzf_resident_bytes(c, bytes, n);
    const int64_t tail = n / LFQ_FA_CHUNK * LFQ_FA_CHUNK;
    if (hipMemsetAsync(d + tail, 0, (size_t)(padded - tail), st) != hipSuccess
        || hipMemcpyAsync(d, res ? res : bytes, (size_t)n, res ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st) != hipSuccess
        || hipStreamSynchronize(st) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    S->times.upload_ms = lfq_now_ms() - t0;
    S->times.n_from_device = res ? 1 : 0;
    if ((rc = S->scan_t.begin(st)) != LFQ_OK) {
        return fail(rc);
    }
    hipLaunchKernelGGL(lfq_fasta_tiles_kernel, dim3((unsigned)V.n_tiles), dim3(LFQ_FA_THREADS), 0, st, V);
    hipLaunchKernelGGL(lfq_fasta_sums_kernel, dim3(1), dim3(LFQ_FA_SCAN_LANES), 0, st, V);
    if (!fa_launched()) {
        return fail(LFQ_ERR_HIP);
    }
    fa->tile_g.resize((size_t)V.n_tiles + 1);
    int64_t tot[2] = {0, 0};
    if (hipMemcpyAsync(fa->tile_g.data(), V.tile_g, (size_t)(V.n_tiles + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess
        || hipMemcpyAsync(&tot[0], V.tile_nl + V.n_tiles, 8, hipMemcpyDeviceToHost, st) != hipSuccess
        || hipMemcpyAsync(&tot[1], V.tile_hd + V.n_tiles, 8, hipMemcpyDeviceToHost, st) != hipSuccess
        || hipStreamSynchronize(st) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    fa->total_graph = fa->tile_g[(size_t)V.n_tiles];
    V.n_lines = 1 + tot[0];
    V.n_hdr = tot[1];
    const int64_t o_hl = lfq_al((V.n_lines + 1) * 8);
    if (hipMalloc((void **)&fa->d_lines, (size_t)(o_hl + lfq_al(std::max<int64_t>(V.n_hdr, 1) * 8))) != hipSuccess) {
        fa->d_lines = nullptr;
        return fail(LFQ_ERR_NOMEM);
    }
    V.lstart = (int64_t *)fa->d_lines;
    V.hline = (int64_t *)(fa->d_lines + o_hl);
    hipLaunchKernelGGL(lfq_fasta_emit_kernel, dim3((unsigned)V.n_tiles), dim3(LFQ_FA_THREADS), 0, st, V);
    if (!fa_launched() || S->scan_t.end(st) != LFQ_OK || hipStreamSynchronize(st) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    S->scan_on = true;
    S->times.n_launches = 3;
    S->times.n_lines = V.n_lines;
    S->times.n_headers = V.n_hdr;
    *out = fa;
    return LFQ_OK;
}

int lfq_fasta_index_build(lfq_fasta *fa, lfq_fasta_index **out, int *why_out, int64_t *bad_line_out, int *bad_byte_out)
{
    int why = LFQ_FA_OK, bad_byte = 0;
    int64_t bad_line = 0;
    auto report = [&]() {
        if (why_out) *why_out = why;
        if (bad_line_out) *bad_line_out = bad_line;
        if (bad_byte_out) *bad_byte_out = bad_byte;
    };
    report();
    if (!fa || !out) {
        return LFQ_ERR_INVALID;
    }
    *out = nullptr;
    lfq_ctx *c = fa->c;
    LfqFastaState *S = fa_state(c);
    const LfqFaView &V = fa->V;
    std::vector<LfqFaRaw> raw((size_t)V.n_hdr);
    std::vector<std::string> names((size_t)V.n_hdr);
    if (V.n > 0) {
        LFQ_TRY_HIP(hipSetDevice(c->device));
        hipStream_t st = c->stream;
        const int64_t nh = std::max<int64_t>(V.n_hdr, 1), o_bad = lfq_al(nh * 8), o_raw = o_bad + lfq_al(8),
                      o_off = o_raw + lfq_al(nh * (int64_t)sizeof(LfqFaRaw)), total = o_off + lfq_al((nh + 1) * 8);
        uint8_t *d = nullptr;
        if (hipMalloc((void **)&d, (size_t)total) != hipSuccess) {
            return LFQ_ERR_NOMEM;
        }
        unsigned long long *seq_m = (unsigned long long *)d, *d_bad = (unsigned long long *)(d + o_bad), bad = FA_NONE;
        LfqFaRaw *d_raw = (LfqFaRaw *)(d + o_raw);
        int64_t *d_off = (int64_t *)(d + o_off);
        uint8_t *d_names = nullptr;
        int rc = LFQ_OK;
        std::vector<int64_t> off((size_t)V.n_hdr + 1, 0);
        std::vector<char> blob;
        if (hipMemsetAsync(d, 0xff, (size_t)(o_bad + 8), st) != hipSuccess || S->lines_t.begin(st) != LFQ_OK) {
            rc = LFQ_ERR_HIP;
            goto done;
        }
        hipLaunchKernelGGL(lfq_fasta_chain_kernel, dim3(fa_grid(V.n_lines)), dim3(256), 0, st, V, seq_m);
        hipLaunchKernelGGL(lfq_fasta_legal_kernel, dim3(fa_grid(V.n_lines)), dim3(256), 0, st, V, seq_m, d_bad);
        S->times.n_launches += 2;
        if (V.n_hdr > 0) {
            hipLaunchKernelGGL(lfq_fasta_entries_kernel, dim3(fa_grid(V.n_hdr)), dim3(256), 0, st, V, seq_m, d_raw);
            S->times.n_launches += 1;
        }
        if (!fa_launched() || S->lines_t.end(st) != LFQ_OK
            || hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st) != hipSuccess
            || (V.n_hdr > 0 && hipMemcpyAsync(raw.data(), d_raw, (size_t)V.n_hdr * sizeof(LfqFaRaw), hipMemcpyDeviceToHost, st) != hipSuccess)
            || hipStreamSynchronize(st) != hipSuccess) {
            rc = LFQ_ERR_HIP;
            goto done;
        }
        S->lines_on = true;
        if (bad != FA_NONE) {
            /* the refusal comes from the smallest (line, why) alone: whatever order the lanes ran in */
            why = (int)(bad & 3);
            bad_line = (int64_t)(bad >> 2) + 1;
            int64_t s = 0;
            uint8_t two[2] = {0, 0};
            if (hipMemcpy(&s, V.lstart + (bad >> 2), 8, hipMemcpyDeviceToHost) != hipSuccess
                || hipMemcpy(two, V.bytes + s, (size_t)std::min<int64_t>(2, V.n - s), hipMemcpyDeviceToHost) != hipSuccess) {
                rc = LFQ_ERR_HIP;
                goto done;
            }
            bad_byte = why == LFQ_FA_UNEXPECTED && two[0] == '\r' ? (s + 1 < V.n ? two[1] : -1) : two[0];
            goto done;
        }
        for (int64_t h = 0; h < V.n_hdr; h++) {
            off[(size_t)h + 1] = off[(size_t)h] + raw[(size_t)h].name_len;
        }
        if (off.back() > 0) {
            blob.resize((size_t)off.back());
            if (hipMalloc((void **)&d_names, (size_t)off.back()) != hipSuccess) {
                d_names = nullptr;
                rc = LFQ_ERR_NOMEM;
                goto done;
            }
            if (hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
                rc = LFQ_ERR_HIP;
                goto done;
            }
            hipLaunchKernelGGL(lfq_fasta_names_kernel, dim3(fa_grid(V.n_hdr)), dim3(256), 0, st, V, d_raw, d_off, d_names);
            S->times.n_launches += 1;
            if (!fa_launched() || hipMemcpyAsync(blob.data(), d_names, blob.size(), hipMemcpyDeviceToHost, st) != hipSuccess
                || hipStreamSynchronize(st) != hipSuccess) {
                rc = LFQ_ERR_HIP;
                goto done;
            }
        }
        for (int64_t h = 0; h < V.n_hdr; h++) {
            names[(size_t)h].assign(blob.data() + off[(size_t)h], (size_t)raw[(size_t)h].name_len);
        }
    done:
        (void)hipStreamSynchronize(st);
        if (d_names) (void)hipFree(d_names);
        (void)hipFree(d);
        if (rc != LFQ_OK) {
            return rc;
        }
        if (why != LFQ_FA_OK) {
            report();
            return LFQ_ERR_INVALID;
        }
    }
    lfq_fasta_index *idx = new lfq_fasta_index();
    why = lfq_fa_entries_finish(raw, names, idx);
    report();
    if (why != LFQ_FA_OK) {
        delete idx;
        return LFQ_ERR_INVALID;
    }
    *out = idx;
    return LFQ_OK;
}

int lfq_fasta_fetch(lfq_fasta *fa, const lfq_fasta_index *idx, const char *name, const lfq_fasta_contig **out)
{
    if (!fa || !idx || !name || !out) {
        return LFQ_ERR_INVALID;
    }
    *out = nullptr;
    const int64_t at = idx->find(name);
    if (at < 0) {
        return LFQ_ERR_INVALID;
    }
    const LfqFaEntry &x = idx->e[(size_t)at];
    lfq_ctx *c = fa->c;
    LfqFastaState *S = fa_state(c);
    const LfqFaView &V = fa->V;
    S->fetch_on = false;
    S->times.fetch_path = LFQ_FASTA_PATH_NONE;
    S->times.n_fetch_bytes = 0;
    S->times.download_ms = 0.0;
    if (x.offset < 0 || x.offset > V.n || x.length < 0 || x.length > fa->total_graph) {
        return LFQ_ERR_INVALID;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    LfqFaFetch F;
    F.offset = x.offset; F.length = x.length; F.blen = x.line_blen; F.llen = x.line_len;
    F.r0 = fa->total_graph;
    if (x.offset < V.n) {
        /* the graph bytes in front of offset: the tile's base and the bytes of the tile in front of it (a copy, no launch) */
        const int64_t t = x.offset / LFQ_FA_TILE, part = x.offset - t * LFQ_FA_TILE;
        uint8_t head[LFQ_FA_TILE];
        if (part > 0) {
            LFQ_TRY_HIP(hipMemcpy(head, V.bytes + t * LFQ_FA_TILE, (size_t)part, hipMemcpyDeviceToHost));
        }
        F.r0 = fa->tile_g[(size_t)t];
        for (int64_t i = 0; i < part; i++) {
            F.r0 += lfq_fa_isgraph(head[i]);
        }
    }
    if (fa->total_graph - F.r0 < x.length) {
        return LFQ_ERR_INVALID;         /* the entry asks for more bases than stand behind its offset */
    }
    if (S->live == fa) {
        S->live = nullptr;              /* the earlier contig goes */
    }
    if (grow(&fa->d_seq, &fa->d_seq_cap, (x.length + 15) / 16 * 16 + 16) != LFQ_OK
        || grow_pinned(&fa->h_seq, &fa->h_seq_cap, x.length + 1) != LFQ_OK) {
        return LFQ_ERR_NOMEM;
    }
    F.out = fa->d_seq;
    if (x.length > 0) {
        const int64_t n_span = F.blen > 0 ? (x.length + F.blen - 1) / F.blen : 0;
        bool regular = F.blen > 0 && F.llen == F.blen + 1
                       && x.offset + (n_span - 1) * F.llen + (x.length - (n_span - 1) * F.blen) <= V.n;
        LFQ_TRY(S->fetch_t.begin(st));
        if (regular) {
            unsigned int *d_flag = (unsigned int *)(fa->d_seq + (x.length + 15) / 16 * 16), flag = 1;
            LFQ_TRY_HIP(hipMemsetAsync(d_flag, 0, 4, st));
            hipLaunchKernelGGL(lfq_fasta_prove_kernel, dim3(fa_grid(n_span)), dim3(256), 0, st, V, F, n_span, d_flag);
            S->times.n_launches += 1;
            if (!fa_launched() || hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st) != hipSuccess
                || hipStreamSynchronize(st) != hipSuccess) {
                return LFQ_ERR_HIP;
            }
            regular = flag == 0;
        }
        const unsigned grid = fa_grid((x.length + 15) / 16);
        if (regular) {
            hipLaunchKernelGGL(lfq_fasta_fetch_regular_kernel, dim3(grid), dim3(256), 0, st, V, F);
        } else {
            hipLaunchKernelGGL(lfq_fasta_fetch_general_kernel, dim3(grid), dim3(256), 0, st, V, F);
        }
        S->times.n_launches += 1;
        S->times.fetch_path = regular ? LFQ_FASTA_PATH_REGULAR : LFQ_FASTA_PATH_GENERAL;
        if (!fa_launched() || S->fetch_t.end(st) != LFQ_OK || hipStreamSynchronize(st) != hipSuccess) {
            return LFQ_ERR_HIP;
        }
        S->fetch_on = true;
        const double t0 = lfq_now_ms();
        LFQ_TRY_HIP(hipMemcpyAsync(fa->h_seq, fa->d_seq, (size_t)x.length, hipMemcpyDeviceToHost, st));
        LFQ_TRY_HIP(hipStreamSynchronize(st));
        S->times.download_ms = lfq_now_ms() - t0;
    }
    fa->h_seq[x.length] = 0;            /* a C string, as faidx_fetch_seq's */
    S->times.n_fetch_bytes = x.length;
    fa->contig.seq = fa->h_seq;
    fa->contig.len = x.length;
    fa->contig.d_seq = fa->d_seq;
    S->live = fa;
    *out = &fa->contig;
    return LFQ_OK;
}

int lfq_last_fasta_times(lfq_ctx *c, lfq_fasta_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    LfqFastaState *S = fa_state(c);
    if (S->scan_on) LFQ_TRY(S->scan_t.ms(&S->times.scan_ms));
    if (S->lines_on) LFQ_TRY(S->lines_t.ms(&S->times.lines_ms));
    if (S->fetch_on) LFQ_TRY(S->fetch_t.ms(&S->times.fetch_ms));
    *t = S->times;
    return LFQ_OK;
}

/* ---- host only: no context ---- */
int lfq_fasta_index_text(const lfq_fasta_index *idx, const char **text, int64_t *n_bytes)
{
    if (!idx || !text || !n_bytes) {
        return LFQ_ERR_INVALID;
    }
    const std::string &s = lfq_fa_index_text(const_cast<lfq_fasta_index *>(idx));   /* (the cached text is not part of its value) */
    *text = s.c_str();
    *n_bytes = (int64_t)s.size();
    return LFQ_OK;
}

int lfq_fasta_index_parse(const char *text, int64_t n_bytes, lfq_fasta_index **out)
{
    if (!out || n_bytes < 0 || (n_bytes > 0 && !text)) {
        return LFQ_ERR_INVALID;
    }
    *out = nullptr;
    lfq_fasta_index *idx = new lfq_fasta_index();
    if (!lfq_fa_index_parse_text(text, n_bytes, idx)) {
        delete idx;
        return LFQ_ERR_INVALID;
    }
    *out = idx;
    return LFQ_OK;
}

void lfq_fasta_index_free(lfq_fasta_index *idx) { delete idx; }
int64_t lfq_fasta_index_n(const lfq_fasta_index *idx) { return idx ? (int64_t)idx->e.size() : 0; }
int64_t lfq_fasta_index_n_duplicates(const lfq_fasta_index *idx) { return idx ? idx->n_dup : 0; }
int64_t lfq_fasta_index_find(const lfq_fasta_index *idx, const char *name) { return idx ? idx->find(name) : -1; }

const char *lfq_fasta_index_name(const lfq_fasta_index *idx, int64_t i)
{
    return idx && i >= 0 && i < (int64_t)idx->e.size() ? idx->e[(size_t)i].name.c_str() : nullptr;
}

int lfq_fasta_index_entry(const lfq_fasta_index *idx, int64_t i, lfq_fasta_entry *entry)
{
    if (!idx || !entry || i < 0 || i >= (int64_t)idx->e.size()) {
        return LFQ_ERR_INVALID;
    }
    const LfqFaEntry &x = idx->e[(size_t)i];
    entry->length = x.length;
    entry->offset = x.offset;
    entry->line_blen = x.line_blen;
    entry->line_len = x.line_len;
    return LFQ_OK;
}

int lfq_checkref(const lfq_fasta_index *idx, const char *const *names, const int64_t *lens, int64_t n, int64_t *first_bad, int *why)
{
    if (first_bad) *first_bad = -1;
    if (why) *why = LFQ_CHECKREF_OK;
    if (!idx || n < 0 || (n > 0 && (!names || !lens))) {
        return LFQ_ERR_INVALID;
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t at = idx->find(names[i]);
        const int bad = at < 0 ? LFQ_CHECKREF_NO_SEQUENCE : idx->e[(size_t)at].length != lens[i] ? LFQ_CHECKREF_LENGTH : LFQ_CHECKREF_OK;
        if (bad != LFQ_CHECKREF_OK) {
            if (first_bad) *first_bad = i;
            if (why) *why = bad;
            return LFQ_OK;
        }
    }
    return LFQ_OK;
}

int lfq_bgzf_gzi_bytes(const lfq_bgzf_result *res, uint8_t *out, int64_t capacity, int64_t *n_bytes)
{
    if (!res || !n_bytes || res->n_blocks < 0 || (res->n_blocks > 0 && (!res->comp_off || !res->data_off))) {
        return LFQ_ERR_INVALID;
    }
    /* as htslib's reader records it while `faidx` walks the file: one entry per read call, which skips empty blocks until one holds
     * data -- the address where the call began (behind the previous block with data) and the uncompressed offset of that block.
     * The first entry, (0, 0), is not written; the empty end-of-file block ends the walk without one */
    std::vector<uint64_t> v(1, 0);
    int64_t prev = -1;
    bool first = true;
    for (int64_t b = 0; b < res->n_blocks; b++) {
        if (res->data_off[b + 1] > res->data_off[b]) {
            if (!first) {
                v.push_back((uint64_t)res->comp_off[prev + 1]);
                v.push_back((uint64_t)res->data_off[b]);
                v[0]++;
            }
            first = false;
            prev = b;
        }
    }
    *n_bytes = (int64_t)v.size() * 8;
    if (out) {
        if (capacity < *n_bytes) {
            return LFQ_ERR_INVALID;
        }
        for (size_t i = 0; i < v.size(); i++) {
            for (int b = 0; b < 8; b++) {
                out[i * 8 + b] = (uint8_t)(v[i] >> (8 * b));
            }
        }
    }
    return LFQ_OK;
}

}
