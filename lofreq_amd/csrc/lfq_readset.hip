/*
 * lfq_readset.hip -- the resident read set: the reads of a region uploaded once; BAQ / IDAQ, source
 * quality and both pileups on the device copy; the host-buffer entry points of those steps around a temporary read set.
 */
#include "lfq_ctx.h"

#include <memory>
#include <queue>

extern "C" {

/* ---- resident read set ------------------------------------------------------------------------------------
 * The reads of one contig region, uploaded once; BAQ / IDAQ, source quality and both pileups work on the device
 * copy and leave their per-base results (lb, ai, ad, sq) there for the next stage.  The host arrays handed to
 * lfq_readset_create stay the caller's and must outlive the read set: the sparse host-side steps (geometry from the
 * CIGARs, the indel event tables) read them in place. */
enum { LFQ_RSC_BLOB = 0, LFQ_RSC_TAGS = 1, LFQ_RSC_PMAX = 2, LFQ_RSC_TAGFL = 3, LFQ_RSC_PINFL = 4, LFQ_RSC_KEEP = 5, LFQ_RSC_IDQ = 6, LFQ_RSC_PINBASES = 7, LFQ_RSC_STORED = 8 };

static bool rs_cache_pinned(int kind)
{
    return kind == LFQ_RSC_PINFL || kind == LFQ_RSC_PINBASES;
}

static void rs_cache_free(int kind, void *p)
{
    if (p) {
        (void)(rs_cache_pinned(kind) ? hipHostFree(p) : hipFree(p));
    }
}

/* `bytes` of device memory (pinned host memory for LFQ_RSC_PINFL and LFQ_RSC_PINBASES): the cached block of this kind if it is large enough */
static void *rs_cache_take(lfq_ctx *c, int kind, size_t bytes, size_t *cap_out)
{
    auto &e = c->rs_cache[kind];
    if (e.p && e.cap >= bytes) {
        void *p = e.p;
        *cap_out = e.cap;
        e.p = nullptr;
        e.cap = 0;
        return p;
    }
    rs_cache_free(kind, e.p);
    e.p = nullptr;
    e.cap = 0;
    void *p = nullptr;
    const size_t want = std::max<size_t>(bytes, 256);
    const hipError_t rc = rs_cache_pinned(kind) ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
    if (rc != hipSuccess) {
        return nullptr;
    }
    *cap_out = want;
    return p;
}

static void rs_cache_give(lfq_ctx *c, int kind, void *p, size_t cap)
{
    if (!p) {
        return;
    }
    auto &e = c->rs_cache[kind];
    if (!e.p || cap > e.cap) {
        rs_cache_free(kind, e.p);
        e.p = p;
        e.cap = cap;
    } else {
        rs_cache_free(kind, p);
    }
}

/* what a read set made by lfq_readset_viterbi or lfq_readset_create_from_bam owns: the host arrays its host-side steps read, in
 * its own read order */
struct LfqReadsetOwned {
    LfqVec<int32_t> pos;
    LfqVec<int64_t> cigar_off, seq_off, order;
    LfqVec<uint32_t> cigar;
    LfqVec<uint8_t> mapq, reverse, flags, seq, qual, bi, bd;
    LfqVec<char> ref;
    uint8_t *pin_bases = nullptr;       /* lfq_readset_create_from_bam: seq | qual | BI | BD as they came back from the device, pinned */
    size_t pin_cap = 0;                 /* (rs_cache kind LFQ_RSC_PINBASES: goes back to the context with the read set) */
};

#define LFQ_UP_CHUNKS 6
struct lfq_readset {
    lfq_ctx *c;
    size_t cap[9];                      /* capacities of blob, tag_blob, d_pmax, d_tagfl, h_fl_pin, d_keep, idq_blob, -, stored_blob
                                           (rs_cache_*; LFQ_RSC_PINBASES: LfqReadsetOwned::pin_cap) */
    int64_t n, n_bases, n_cig, ref_len;
    const int32_t *pos;
    const int64_t *cigar_off, *seq_off;
    const uint32_t *cigar;
    const uint8_t *seq, *qual, *mapq, *reverse;
    const char *ref;
    const uint8_t *h_bi, *h_bd, *h_ai, *h_ad, *h_flags;     /* tag bytes on the host, as given (may be null) */
    const int32_t *h_sq;
    uint8_t *blob, *tag_blob;           /* inputs; lb / ai / ad computed by lfq_readset_baq */
    uint8_t *d_pos, *d_coff, *d_soff, *d_cig, *d_seq, *d_qual, *d_ref, *d_mapq, *d_rev, *d_bi, *d_bd, *d_lb, *d_ai,
            *d_ad, *d_fl, *d_sqb;
    bool has_lb, has_idaq, has_sqb, has_bi, has_bd;
    /* lfq_readset_indelqual: BI / BD computed here (d_bi / d_bd then point into idq_blob, every read has both tags, and the
     * host side of the indel pileup evaluates the bytes it needs instead of reading h_bi / h_bd) */
    int idq_mode;                       /* 0: not run; LFQ_IDQ_UNIFORM / LFQ_IDQ_DINDEL */
    uint8_t idq_ins, idq_del;           /* uniform mode: the two tag bytes */
    uint8_t *idq_blob;                  /* BI | BD (uniform) or the one string both are (Dindel) | the position table */
    hipEvent_t ev_idq;                  /* its kernels are done: the pileup may run on another stream */
    std::vector<uint8_t> fl;            /* per read: bit 0..3 = has BI / BD / ai / ad (host flags or from the device BAQ) */
    std::vector<int32_t> sq32;          /* source quality per read once computed */
    /* lfq_readset_baq returns when its kernels are queued: what follows on the device is ordered by the stream, what the
     * host needs (which reads got an ai / ad tag) arrives in pinned memory and is picked up by readset_baq_wait */
    uint8_t *d_tagfl, *h_fl_pin;        /* [n] bit 0: ai, bit 1: ad written by the kernels; [n] merged flags on their way back */
    hipEvent_t ev_baq;
    bool baq_pending, baq_idaq;
    int32_t *d_pmax;                    /* position-sorted reads: running maximum of the end coordinates (lazily) */
    int pmax_state;                     /* 0 unknown, 1 sorted (d_pmax valid), 2 unsorted, LFQ_ERR_NOMEM / LFQ_ERR_HIP: sorted, but d_pmax
                                         * could not be made */
    /* -d cap (lfq_set_max_depth): the reads both pileups take, decided once per cap value (readset_keep) */
    bool keep_valid;                    /* a decision for the cap keep_for has been made; keep_rc is its result */
    int64_t keep_for;
    int keep_rc;                        /* LFQ_OK, or LFQ_ERR_INVALID for reads that are not position-sorted */
    int64_t n_kept;
    std::vector<uint8_t> keep;          /* [n] 1 = kept; empty when the cap drops nothing (the pileups then run as without it) */
    std::vector<int32_t> keep_end;      /* [n] exclusive end of every read (with a mask: what the compaction kernels take) */
    uint8_t *d_keep;                    /* device: the mask, the kept reads' read_idx / pos / pmax_end, compaction scratch */
    bool keep_dev_valid;                /* d_keep holds the kept reads of the decision for keep_dev_for */
    int64_t keep_dev_for;
    hipEvent_t ev_keep;                 /* the compaction kernels are done (the two pileups may run on different streams) */
    /* lfq_readset_create returns while the reads are still crossing PCIe (a helper thread feeds the copies of the caller's
     * pageable arrays to the upload stream): host-only work of the next step -- the BAQ geometry -- runs meanwhile, and
     * every step calls readset_upload_wait before its first device operation on the read set */
    std::thread *up_thread;
    std::atomic<int> up_stage;          /* 1: everything but BI / BD has landed (what lfq_readset_baq reads), 2: all of it */
    std::atomic<int> up_chunks;         /* bases + qualities of the reads [0, up_bound[up_chunks]) have landed */
    int up_nchunks;
    int64_t up_bound[LFQ_UP_CHUNKS + 1]; /* chunk j = reads [up_bound[j], up_bound[j + 1]); the first ones are small: 1, 2, 4
                                          * rounds of the BAQ kernel over the SIMDs, so that its first launch starts early */
    std::atomic<int> up_rc;        /* written by the helper thread at the end of each stage */
    LfqPin<uint8_t> *up_fl;             /* the flag bytes on their way out (pinned; handed back once the copies are done) */
    /* Pinned caller arrays (lfq_host_alloc): the copies are DMA transfers queued by lfq_readset_create itself, and what
     * waits for them is a STREAM, not the host -- events instead of the helper thread's progress counters */
    bool up_events;
    hipEvent_t ev_chunk[LFQ_UP_CHUNKS]; /* bases + qualities of the reads up to chunk j have landed */
    hipEvent_t ev_stage[2];             /* [0]: everything but BI / BD, [1]: all of it */
    LfqReadsetOwned *own;               /* lfq_readset_viterbi's result: the host views above point into it (else null) */
    /* lfq_readset_create_from_bam_tags: the first lb / ai / ad strings the records carry, waiting for lfq_readset_baq_fill */
    std::vector<uint8_t> stored_fl;     /* [n] bit 0 / 1 / 2: lb / ai / ad stored; empty: no read has a stored tag */
    std::vector<uint8_t> take;          /* [n] the last fill's merge mask, as it went to d_take */
    uint8_t *stored_blob;               /* take[n] | lb | ai | ad, the arrays of the tags a read has */
    uint8_t *d_take, *d_st[3];          /* (d_st[t] null: no read has tag t) */
    bool filled;                        /* the resident lb / ai / ad hold stored bytes: no longer what `alnqual` would append */
    /* -l targets (lfq_set_bed): the context's table when the read set was created (a reference; null: none), and which reads
     * overlap it -- decided once, on the device (readset_bed_keep) */
    LfqBedDev *bed;
    bool bed_valid;
    int bed_rc;
    std::vector<uint8_t> bed_keep;      /* [n] 1 = the read overlaps an interval */
    int64_t n_bed_kept;
    bool ref_from_device;               /* the contig came from the context's live lfq_fasta_fetch result, device to device */
};

/* the reads, qualities, CIGARs and the contig are on the device (BI / BD may still be on their way: the BAQ kernels do
 * not read them, and 600 of the 1300 MB of a 2 M-read region then cross PCIe under those kernels).  Every one of the three
 * waits below makes the given stream(s) wait when the uploads are tracked by events, and the host otherwise. */
static int readset_upload_wait_inputs(lfq_readset *rs, std::initializer_list<hipStream_t> streams)
{
    if (rs && rs->up_events) {
        for (hipStream_t st : streams) {
            if (st && hipStreamWaitEvent(st, rs->ev_stage[0], 0) != hipSuccess) {
                return LFQ_ERR_HIP;
            }
        }
        return LFQ_OK;
    }
    if (rs && rs->up_thread) {
        while (rs->up_stage.load(std::memory_order_acquire) < 1) {
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        return rs->up_rc;
    }
    return rs ? rs->up_rc.load() : (int)LFQ_OK;
}

/* ... and for a launch over the reads up to (and including) r_last: the small arrays and the chunks of bases and
 * qualities that hold them */
static int readset_upload_wait_reads(lfq_readset *rs, int64_t r_last, hipStream_t st)
{
    if (rs && (rs->up_thread || rs->up_events)) {
        int need = 1;
        while (need < rs->up_nchunks && rs->up_bound[need] <= r_last) {
            need++;
        }
        if (rs->up_events) {
            return hipStreamWaitEvent(st, rs->ev_chunk[need - 1], 0) == hipSuccess ? (int)LFQ_OK : (int)LFQ_ERR_HIP;
        }
        while (rs->up_chunks.load(std::memory_order_acquire) < need) {
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
    return rs ? rs->up_rc.load() : (int)LFQ_OK;
}

/* all of it.  st = null: the host waits (and the pinned flag bytes go back to the pool) */
static int readset_upload_wait(lfq_readset *rs, hipStream_t st = nullptr)
{
    if (rs && rs->up_events) {
        if (st) {
            return hipStreamWaitEvent(st, rs->ev_stage[1], 0) == hipSuccess ? (int)LFQ_OK : (int)LFQ_ERR_HIP;
        }
        if (hipEventSynchronize(rs->ev_stage[1]) != hipSuccess) {
            return LFQ_ERR_HIP;
        }
    }
    if (rs && rs->up_thread) {
        rs->up_thread->join();
        delete rs->up_thread;
        rs->up_thread = nullptr;
    }
    if (rs && rs->up_fl) {
        delete rs->up_fl;
        rs->up_fl = nullptr;
    }
    return rs ? rs->up_rc.load() : (int)LFQ_OK;
}

/* the host side of an lfq_readset_baq that is still running: merged tag flags (bit 0 BI, 1 BD, 2 ai, 3 ad) into rs->fl */
static int readset_baq_wait(lfq_readset *rs)
{
    if (!rs || !rs->baq_pending) {
        return LFQ_OK;
    }
    rs->baq_pending = false;
    if (hipEventSynchronize(rs->ev_baq) != hipSuccess) {
        return LFQ_ERR_HIP;
    }
    if (rs->baq_idaq && rs->h_fl_pin) {
        memcpy(rs->fl.data(), rs->h_fl_pin, (size_t)rs->n);
    }
    return LFQ_OK;
}

void lfq_readset_destroy(lfq_readset *rs)
{
    if (rs) {
        (void)readset_upload_wait(rs);
        (void)readset_baq_wait(rs);
        if (rs->ev_baq) (void)hipEventDestroy(rs->ev_baq);
        (void)hipStreamSynchronize(rs->c->stream);      /* nothing queued may still use what goes back to the cache */
        for (hipEvent_t e : {rs->ev_chunk[0], rs->ev_chunk[1], rs->ev_chunk[2], rs->ev_chunk[3], rs->ev_chunk[4], rs->ev_chunk[5],
                             rs->ev_stage[0], rs->ev_stage[1]}) {
            if (e) (void)hipEventDestroy(e);
        }
        rs_cache_give(rs->c, LFQ_RSC_PINFL, rs->h_fl_pin, rs->cap[LFQ_RSC_PINFL]);
        rs_cache_give(rs->c, LFQ_RSC_TAGFL, rs->d_tagfl, rs->cap[LFQ_RSC_TAGFL]);
        rs_cache_give(rs->c, LFQ_RSC_BLOB, rs->blob, rs->cap[LFQ_RSC_BLOB]);
        rs_cache_give(rs->c, LFQ_RSC_TAGS, rs->tag_blob, rs->cap[LFQ_RSC_TAGS]);
        rs_cache_give(rs->c, LFQ_RSC_PMAX, rs->d_pmax, rs->cap[LFQ_RSC_PMAX]);
        rs_cache_give(rs->c, LFQ_RSC_KEEP, rs->d_keep, rs->cap[LFQ_RSC_KEEP]);
        if (rs->ev_idq) {
            (void)hipEventSynchronize(rs->ev_idq);      /* (its stream need not be c->stream) */
            (void)hipEventDestroy(rs->ev_idq);
        }
        rs_cache_give(rs->c, LFQ_RSC_IDQ, rs->idq_blob, rs->cap[LFQ_RSC_IDQ]);
        rs_cache_give(rs->c, LFQ_RSC_STORED, rs->stored_blob, rs->cap[LFQ_RSC_STORED]);
        if (rs->ev_keep) (void)hipEventDestroy(rs->ev_keep);
        if (rs->own) {
            rs_cache_give(rs->c, LFQ_RSC_PINBASES, rs->own->pin_bases, rs->own->pin_cap);
        }
        lfq_bed_dev_release(rs->bed);
        delete rs->own;
        delete rs;
    }
}

/* lfq_readset_create; rd->seq may be null here (lfq_indelqual_batch: its kernels read no bases).  take_bed: the read set takes the
 * context's targets (lfq_set_bed) -- every read set a caller sees does; those behind lfq_baq_batch and lfq_indelqual_batch, the
 * library's `alnqual` and `indelqual`, which have no -l, do not.  bases_resident
 * (lfq_readset_viterbi): the per-base device arrays -- seq, qual, BI, BD -- get their room but no copy; the caller fills them
 * on the device before it hands the read set out */
static int readset_create(lfq_ctx *c, const lfq_pileup_reads *rd, const lfq_pileup_indel_tags *tg, lfq_readset **out,
                          bool bases_resident = false, bool take_bed = true)
{
    if (!c || !rd || !out || rd->n_reads < 0
        || (rd->n_reads > 0 && (!rd->pos || !rd->cigar_off || !rd->cigar || !rd->seq_off || !rd->ref))) {
        return LFQ_ERR_INVALID;
    }
    *out = nullptr;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    lfq_readset *rs = new lfq_readset();
    rs->c = c;
    rs->n = rd->n_reads;
    rs->n_bases = rs->n > 0 ? rd->seq_off[rs->n] : 0;
    rs->n_cig = rs->n > 0 ? rd->cigar_off[rs->n] : 0;
    rs->ref_len = rd->ref_len;
    rs->pos = rd->pos; rs->cigar_off = rd->cigar_off; rs->seq_off = rd->seq_off; rs->cigar = rd->cigar;
    rs->seq = rd->seq; rs->qual = rd->qual; rs->mapq = rd->mapq; rs->reverse = rd->reverse; rs->ref = rd->ref;
    rs->h_bi = tg ? tg->bi : nullptr; rs->h_bd = tg ? tg->bd : nullptr;
    rs->h_ai = tg ? tg->ai : nullptr; rs->h_ad = tg ? tg->ad : nullptr;
    rs->h_flags = tg ? tg->tag_flags : nullptr;
    rs->h_sq = tg ? tg->sq : nullptr;
    rs->blob = nullptr;
    rs->tag_blob = nullptr;
    rs->d_pmax = nullptr;
    rs->d_tagfl = nullptr;
    rs->h_fl_pin = nullptr;
    memset(rs->cap, 0, sizeof(rs->cap));
    rs->pmax_state = 0;
    rs->keep_valid = rs->keep_dev_valid = false;
    rs->d_keep = nullptr;
    rs->ev_keep = nullptr;
    rs->idq_mode = 0;
    rs->idq_blob = nullptr;
    rs->ev_idq = nullptr;
    rs->up_thread = nullptr;
    rs->up_stage.store(0);
    rs->up_chunks.store(0);
    rs->up_nchunks = 1;
    rs->up_rc = LFQ_OK;
    rs->up_fl = nullptr;
    rs->own = nullptr;
    rs->stored_blob = rs->d_take = rs->d_st[0] = rs->d_st[1] = rs->d_st[2] = nullptr;
    rs->filled = false;
    rs->bed = take_bed ? lfq_bed_dev_retain(c->bed) : nullptr;
    rs->bed_valid = false;
    rs->bed_rc = LFQ_OK;
    rs->n_bed_kept = 0;
    rs->ref_from_device = false;
    rs->has_lb = rs->has_idaq = rs->has_sqb = rs->has_bi = rs->has_bd = false;
    const int64_t n = rs->n, nb = rs->n_bases;
    {
        const uint32_t have = (rs->h_bi ? 1u : 0u) | (rs->h_bd ? 2u : 0u) | (rs->h_ai ? 4u : 0u) | (rs->h_ad ? 8u : 0u);
        rs->fl.assign((size_t)std::max<int64_t>(n, 1), (uint8_t)have);      /* no per-read flags: every read has every tag given */
        for (int64_t r = 0; rs->h_flags && r < n; r++) {
            rs->fl[(size_t)r] = (uint8_t)(rs->h_flags[r] & have);
        }
    }
    if (n == 0) {
        *out = rs;
        return LFQ_OK;
    }
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t o = off; off += lfq_al(bytes); return o; };
    /* per-base arrays only where there is something to put: device allocations of this size are not free.  The
     * outputs of lfq_readset_baq (lb, ai, ad) get their own allocation when that step runs. */
    const int64_t o_pos = take(n * 4), o_coff = take((n + 1) * 8), o_soff = take((n + 1) * 8), o_cig = take(rs->n_cig * 4),
                  o_seq = take(rd->seq ? nb + 16 : 0), o_qual = take(rd->qual ? nb + 16 : 0), o_ref = take(rs->ref_len + 1), o_mapq = take(n),
                  o_rev = take(n), o_bi = take(rs->h_bi ? nb + 16 : 0), o_bd = take(rs->h_bd ? nb + 16 : 0),
                  o_lb = take(rd->baq ? nb + 16 : 0), o_fl = take(n), o_sqb = take(n);
    rs->blob = (uint8_t *)rs_cache_take(c, LFQ_RSC_BLOB, (size_t)off, &rs->cap[LFQ_RSC_BLOB]);
    if (!rs->blob) {
        lfq_bed_dev_release(rs->bed);
        delete rs;
        return LFQ_ERR_NOMEM;
    }
    uint8_t *d = rs->blob;
    rs->d_pos = d + o_pos; rs->d_coff = d + o_coff; rs->d_soff = d + o_soff; rs->d_cig = d + o_cig; rs->d_seq = d + o_seq;
    rs->d_qual = d + o_qual; rs->d_ref = d + o_ref; rs->d_mapq = d + o_mapq; rs->d_rev = d + o_rev; rs->d_bi = d + o_bi;
    rs->d_bd = d + o_bd; rs->d_lb = rd->baq ? d + o_lb : nullptr; rs->d_ai = nullptr; rs->d_ad = nullptr; rs->d_fl = d + o_fl;
    rs->d_sqb = d + o_sqb;
    if (!c->up_stream && hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking) != hipSuccess) {
        c->up_stream = nullptr;
        lfq_readset_destroy(rs);
        return LFQ_ERR_HIP;
    }
    rs->up_fl = new LfqPin<uint8_t>(c, (size_t)n);       /* not from rs->fl: see LfqPin */
    if (!rs->up_fl->ok()) {
        lfq_readset_destroy(rs);
        return LFQ_ERR_NOMEM;
    }
    memcpy(rs->up_fl->data(), rs->fl.data(), (size_t)n);
    /* The order of the copies follows what lfq_readset_baq, usually the first step, needs: the small per-read arrays, then
     * bases and qualities in chunks of reads -- its launch over reads [a, b) starts when the chunks up to read b have
     * landed (readset_upload_wait_reads) --, BI / BD, which it does not read, last. */
    struct Copy { uint8_t *dst; const void *src; int64_t bytes; int chunks_after, stage_after; bool from_device; };
    std::vector<Copy> todo;
    int64_t up_bytes = 0;
    auto add = [&](uint8_t *dst, const void *src, int64_t bytes) {
        if (src && bytes > 0) {
            todo.push_back({dst, src, bytes, 0, 0, false});
            up_bytes += bytes;
        }
    };
    add(rs->d_pos, rd->pos, n * 4);
    add(rs->d_coff, rd->cigar_off, (n + 1) * 8);
    add(rs->d_soff, rd->seq_off, (n + 1) * 8);
    add(rs->d_cig, rd->cigar, rs->n_cig * 4);
    add(rs->d_ref, rd->ref, rs->ref_len);
    /* a contig that lfq_fasta_fetch left resident does not cross the link again */
    if (const uint8_t *d_res = rs->ref_len > 0 ? lfq_fasta_resident(c, (const uint8_t *)rd->ref, rs->ref_len) : nullptr) {
        todo.back().src = d_res;
        todo.back().from_device = true;
        up_bytes -= rs->ref_len;
        rs->ref_from_device = true;
    }
    add(rs->d_mapq, rd->mapq, n);
    add(rs->d_rev, rd->reverse, n);
    add(rs->d_lb, rd->baq, nb);
    add(rs->d_sqb, rd->sq, n);
    add(rs->d_fl, rs->up_fl->data(), n);
    /* chunks of reads: small first ones -- the reads of one round of the BAQ register kernel over the SIMDs (one wavefront
     * of 64 reads each), what lfq_readset_baq's first launch takes, then two and four -- and the rest in equal parts */
    const int64_t first_reads = (int64_t)c->n_cu * 4 * 64;
    const int n_chunks = nb >= ((int64_t)64 << 20) ? (n >= 16 * first_reads ? LFQ_UP_CHUNKS : 4) : 1;
    rs->up_nchunks = n_chunks;
    rs->up_bound[0] = 0;
    if (n_chunks == LFQ_UP_CHUNKS) {
        /* 1, 2, 4 rounds (the link delivers reads about twice as fast as the kernel takes them: while a launch runs, the
         * reads of one twice its size arrive), the rest in three equal parts */
        rs->up_bound[1] = first_reads;
        rs->up_bound[2] = 3 * first_reads;
        rs->up_bound[3] = 7 * first_reads;
        for (int j = 4; j <= n_chunks; j++) {
            rs->up_bound[j] = 7 * first_reads + (n - 7 * first_reads) * (j - 3) / (n_chunks - 3);
        }
    } else {
        for (int j = 1; j <= n_chunks; j++) {
            rs->up_bound[j] = n * j / n_chunks;
        }
    }
    for (int j = 0; j < n_chunks; j++) {
        const int64_t b0 = rd->seq_off[rs->up_bound[j]], b1 = rd->seq_off[rs->up_bound[j + 1]];
        add(rs->d_seq + b0, rd->seq && !bases_resident ? rd->seq + b0 : nullptr, b1 - b0);
        add(rs->d_qual + b0, rd->qual && !bases_resident ? rd->qual + b0 : nullptr, b1 - b0);
        if (!todo.empty()) {
            todo.back().chunks_after = j + 1;
        }
    }
    if (!todo.empty()) {
        todo.back().stage_after = 1;
    }
    add(rs->d_bi, bases_resident ? nullptr : rs->h_bi, nb);
    add(rs->d_bd, bases_resident ? nullptr : rs->h_bd, nb);
    if (!todo.empty()) {
        todo.back().stage_after = 2;
    }
    rs->has_bi = rs->h_bi != nullptr;
    rs->has_bd = rs->h_bd != nullptr;
    rs->has_lb = rd->baq != nullptr;
    rs->has_sqb = rd->sq != nullptr;
    const int device = c->device;
    hipStream_t ups = c->up_stream;
    auto run = [rs, todo, n_chunks, device, ups]() {
        int rc = hipSetDevice(device) == hipSuccess ? LFQ_OK : LFQ_ERR_HIP;
        for (const Copy &x : todo) {
            if (rc == LFQ_OK && hipMemcpyAsync(x.dst, x.src, (size_t)x.bytes, x.from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ups) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
            if (x.chunks_after || x.stage_after) {      /* progress is published when the copies have landed */
                if (hipStreamSynchronize(ups) != hipSuccess && rc == LFQ_OK) {
                    rc = LFQ_ERR_HIP;
                }
                rs->up_rc = rc;
                if (x.chunks_after) {
                    rs->up_chunks.store(x.chunks_after, std::memory_order_release);
                }
                if (x.stage_after) {
                    rs->up_stage.store(x.stage_after, std::memory_order_release);
                }
            }
        }
        rs->up_rc = rc;
        rs->up_chunks.store(n_chunks, std::memory_order_release);
        rs->up_stage.store(2, std::memory_order_release);
    };
    const int up_mode = lfq_knobs().sync_upload;        /* 0: helper thread from 8 MB on, 1: never, 2: always */
    if (up_mode == 0 && up_bytes >= ((int64_t)8 << 20) && lfq_is_pinned(rd->seq) && lfq_is_pinned(rd->qual)
        && lfq_is_pinned(rs->h_bi) && lfq_is_pinned(rs->h_bd)) {
        /* the big arrays are pinned: every copy is queued right here (the small pageable ones, if any, are staged by the
         * runtime inside the call), events mark the stages, and nothing on the host ever waits for the link */
        int rc = LFQ_OK;
        for (int j = 0; j < LFQ_UP_CHUNKS + 2 && rc == LFQ_OK; j++) {
            hipEvent_t *e = j < LFQ_UP_CHUNKS ? &rs->ev_chunk[j] : &rs->ev_stage[j - LFQ_UP_CHUNKS];
            if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
        }
        bool stage0_done = false;
        for (const Copy &x : todo) {
            if (rc == LFQ_OK && hipMemcpyAsync(x.dst, x.src, (size_t)x.bytes, x.from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ups) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
            if (rc == LFQ_OK && x.chunks_after && hipEventRecord(rs->ev_chunk[x.chunks_after - 1], ups) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
            if (rc == LFQ_OK && x.stage_after && hipEventRecord(rs->ev_stage[x.stage_after - 1], ups) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
            if (rc == LFQ_OK && x.stage_after == 2 && !stage0_done && hipEventRecord(rs->ev_stage[0], ups) != hipSuccess) {
                rc = LFQ_ERR_HIP;           /* (no BI / BD: the last copy ends both stages) */
            }
            stage0_done = stage0_done || x.stage_after != 0;
        }
        for (int j = n_chunks; j < LFQ_UP_CHUNKS && rc == LFQ_OK; j++) {   /* fewer chunks than events: the unused ones are the last one */
            if (hipEventRecord(rs->ev_chunk[j], ups) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
        }
        if (rc != LFQ_OK) {
            (void)hipStreamSynchronize(ups);
            lfq_readset_destroy(rs);
            return rc;
        }
        rs->up_events = true;
        rs->up_rc = LFQ_OK;
        rs->up_chunks.store(n_chunks, std::memory_order_release);
        rs->up_stage.store(2, std::memory_order_release);
    } else if (up_mode == 2 || (up_bytes >= ((int64_t)8 << 20) && up_mode == 0)) {
        rs->up_thread = new std::thread(run);           /* readset_upload_wait joins it */
    } else {
        run();
        const int rc = readset_upload_wait(rs);
        if (rc != LFQ_OK) {
            lfq_readset_destroy(rs);
            return rc;
        }
    }
    *out = rs;
    return LFQ_OK;
}

int lfq_readset_create(lfq_ctx *c, const lfq_pileup_reads *rd, const lfq_pileup_indel_tags *tg, lfq_readset **out)
{
    if (rd && rd->n_reads > 0 && !rd->seq) {
        return LFQ_ERR_INVALID;
    }
    return readset_create(c, rd, tg, out);
}

/* Reads that are not position-sorted: the column-major kernels cannot take them (no window to search), the read-major ones hand
 * a column's observations out in the order their threads get there (an atomic cursor), so that the last bits of a p-value can
 * differ from run to run.  The reference cannot take such input at all (bam_mplp_auto needs a coordinate-sorted file,
 * plp.c:1406-1447): refused unless the caller asked for it (lfq_set_pileup_unsorted; the tuning build's LFQ_PILEUP_ATOMIC sends
 * even sorted reads that way, for the tests that hold the two kernel families against each other). */
static bool readset_unsorted_ok(const lfq_ctx *c)
{
    return c->plp_unsorted_ok || lfq_knobs().pileup_atomic;
}

/* position-sorted reads (what mpileup requires) take the column-major pileup kernels, which find the reads that can
 * overlap a position by binary search: they need the running maximum of the end coordinates, rs->d_pmax (made on the first
 * call, its upload waited for on `st`; null: the reads are not sorted).  -> LFQ_ERR_INVALID for unsorted reads, unless the entry
 * can take them at all (unsorted_may: the two region pileups, which have read-major kernels) and the caller asked for it */
static int readset_pmax(lfq_ctx *c, lfq_readset *rs, hipStream_t st, bool unsorted_may)
{
    if (rs->pmax_state == 0) {
        rs->pmax_state = 2;
        const int64_t n = rs->n;
        LfqPin<int32_t> pmax(c, (size_t)std::max<int64_t>(n, 1));
        const bool wanted = !lfq_knobs().pileup_atomic && n > 0;
        if (wanted && !pmax.ok()) {
            rs->pmax_state = LFQ_ERR_NOMEM;
        }
        if (wanted && pmax.ok()) {
            /* two passes split over a few threads: end coordinate and running maximum inside a part (and whether the
             * part is sorted), then the maximum of the parts before it */
            int32_t part_max[LFQ_HOST_PARTS];
            bool part_sorted[LFQ_HOST_PARTS];
            int parts = 1;
            lfq_for_reads(n, [&](int64_t r0, int64_t r1, int part) {
                int32_t run = INT32_MIN;
                bool sorted = true;
                for (int64_t r = r0; r < r1; r++) {
                    const uint32_t *cg = rs->cigar + rs->cigar_off[r];
                    const int nc = (int)(rs->cigar_off[r + 1] - rs->cigar_off[r]);
                    int64_t e = rs->pos[r];
                    for (int k = 0; k < nc; k++) {
                        const int op = cg[k] & 0xf;
                        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) {
                            e += cg[k] >> 4;
                        }
                    }
                    run = std::max<int32_t>(run, (int32_t)std::min<int64_t>(e, INT32_MAX));
                    pmax[(size_t)r] = run;
                    sorted = sorted && (r == 0 || rs->pos[r] >= rs->pos[r - 1]);     /* r0 - 1 belongs to the part before */
                }
                part_max[part] = run;
                part_sorted[part] = sorted;
            }, &parts);
            bool sorted = true;
            for (int q = 0; q < parts; q++) {
                sorted = sorted && part_sorted[q];
            }
            if (sorted && parts > 1) {
                int32_t before[LFQ_HOST_PARTS];
                before[0] = INT32_MIN;
                for (int q = 1; q < parts; q++) {
                    before[q] = std::max(before[q - 1], part_max[q - 1]);
                }
                lfq_for_reads(n, [&](int64_t r0, int64_t r1, int part) {
                    const int32_t m = before[part];
                    for (int64_t r = r0; r < r1 && pmax[(size_t)r] < m; r++) {     /* the running maximum only grows */
                        pmax[(size_t)r] = m;
                    }
                });
            }
            if (sorted) {
                rs->d_pmax = (int32_t *)rs_cache_take(c, LFQ_RSC_PMAX, (size_t)n * 4, &rs->cap[LFQ_RSC_PMAX]);
                if (rs->d_pmax
                    && hipMemcpyAsync(rs->d_pmax, pmax.data(), (size_t)n * 4, hipMemcpyHostToDevice, st) == hipSuccess
                    && hipStreamSynchronize(st) == hipSuccess) {
                    rs->pmax_state = 1;
                } else if (rs->d_pmax) {
                    rs->pmax_state = LFQ_ERR_HIP;
                    rs_cache_give(c, LFQ_RSC_PMAX, rs->d_pmax, rs->cap[LFQ_RSC_PMAX]);
                    rs->d_pmax = nullptr;
                } else {
                    rs->pmax_state = LFQ_ERR_NOMEM;
                }
            }
        }
    }
    if (rs->pmax_state < 0) {
        return rs->pmax_state;
    }
    return rs->d_pmax || rs->n == 0 || (unsorted_may && readset_unsorted_ok(c)) ? (int)LFQ_OK : (int)LFQ_ERR_INVALID;
}

/* ---- -l / --bed (lfq_set_bed) -----------------------------------------------------------------------------------
 * plp.c:625-629: a read that overlaps no interval of the targets is dropped behind the flag filters and in front of BAQ and of
 * bam_plp_push.  Which reads those are is decided once per read set, by lfq_bed_keep_kernel on the start positions and CIGAR words
 * the read set has on the device; the bytes come back once (a byte a read), because the two things that follow are made on the
 * host: the launch lists of the HMM kernels (readset_baq_run) and the -d rule on the survivors (readset_keep).  The kernel goes to
 * the context's stream behind the first chunk of the upload, which the small per-read arrays are in front of; the mask lands in
 * the context's BAQ temporary, which the same stream fills again when the BAQ step runs. */
static int readset_bed_keep(lfq_ctx *c, lfq_readset *rs)
{
    if (!rs->bed || rs->bed_valid) {
        return rs->bed_rc;
    }
    rs->bed_valid = true;
    const int64_t n = rs->n;
    rs->n_bed_kept = 0;
    if (n == 0) {
        return LFQ_OK;
    }
    auto run = [&]() -> int {
        LFQ_TRY_HIP(hipSetDevice(c->device));
        LFQ_TRY(readset_upload_wait_reads(rs, 0, c->stream));
        LfqPin<uint8_t> h(c, (size_t)n);
        LFQ_PIN_OK(h);
        if (rs->bed->tab.n > 0) {
            LFQ_TRY(grow(&c->d_tmp[0], &c->tmp_bytes[0], n));
            uint8_t *d_mask = c->d_tmp[0];
            int rc = lfq_launch_bed_keep(rs->bed->tab, (const int32_t *)rs->d_pos, (const int64_t *)rs->d_coff,
                                         (const uint32_t *)rs->d_cig, n, d_mask, c->stream);
            if (rc == LFQ_OK && hipMemcpyAsync(h.data(), d_mask, (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
            if (hipStreamSynchronize(c->stream) != hipSuccess && rc == LFQ_OK) {
                rc = LFQ_ERR_HIP;
            }
            LFQ_TRY(rc);
        } else {
            memset(h.data(), 0, (size_t)n);         /* an empty table: nothing overlaps, nothing to launch */
        }
        rs->bed_keep.assign(h.data(), h.data() + n);
        int64_t kept = 0;
        for (int64_t r = 0; r < n; r++) {
            kept += rs->bed_keep[(size_t)r];
        }
        rs->n_bed_kept = kept;
        return LFQ_OK;
    };
    rs->bed_rc = run();
    return rs->bed_rc;
}

/* ---- -d / --max-depth (lfq_set_max_depth) --------------------------------------------------------------------
 * htslib's bam_plp_push does not push a read that starts at the iterator's current position while its node pool holds more
 * than maxcnt reads (bam_mplp_set_maxcnt, plp.c:1391-1392).  On the reads in file order: the first read at a start position P
 * is always kept, every later one is dropped when at least max_depth KEPT reads before it have an exclusive end >= P.  A
 * recurrence over the start positions, sequential by nature -- so the host decides, once per read set and cap value, and the
 * device gets a compacted read list (lfq_launch_keep_compact).
 *   1. ends and the running maximum of the ends, split over the lfq_for_reads threads (as readset_pmax);
 *   2. the proof, over the runs of equal start in parallel: if every read were kept, at most (end of the run) - (first read
 *      whose running maximum reaches P) reads would count at the last read of a run at P.  Within the cap at every run:
 *      nothing is dropped, no mask, the pileups run exactly as without a cap;
 *   3. otherwise one walk over the reads with a min-heap of the kept reads' ends (reads * log depth).
 * With targets (lfq_set_bed) the reads bam_plp_push sees are those the BED leaves (readset_bed_keep), in file order: the mask starts
 * from them, the proof of step 2 holds for a subset of the reads it counts, and the walk of step 3 passes over the others.  Without
 * a cap the mask is the BED's, and reads that are not position-sorted are fine (no rule on file order is applied). */
static bool readset_masked(const lfq_ctx *c, const lfq_readset *rs)
{
    return c->plp_max_depth != LFQ_NO_MAX_DEPTH || rs->bed != nullptr;
}

static int readset_keep(lfq_ctx *c, lfq_readset *rs)
{
    const int64_t md = c->plp_max_depth;
    if (!readset_masked(c, rs)) {
        return LFQ_OK;
    }
    LFQ_TRY(readset_bed_keep(c, rs));
    const uint8_t *bk = rs->bed && rs->n > 0 ? rs->bed_keep.data() : nullptr;
    if (rs->keep_valid && rs->keep_for == md) {
        return rs->keep_rc;
    }
    if (rs->keep_dev_valid) {
        /* the cap changed between the pileups of this read set: the kernels of the earlier pileup may still read the kept-read
         * list (and the copies its mask and ends came from), on either of the two streams the pileups use -- both drain before
         * any of it is rewritten */
        LFQ_TRY_HIP(hipStreamSynchronize(c->stream));
        if (c->dps) LFQ_TRY_HIP(hipStreamSynchronize(c->dps));
        rs->keep_dev_valid = false;
    }
    rs->keep_valid = true;
    rs->keep_for = md;
    rs->keep_rc = LFQ_OK;
    rs->keep.clear();
    rs->keep_end.clear();
    const int64_t n = rs->n;
    rs->n_kept = n;
    if (n == 0) {
        return LFQ_OK;
    }
    std::vector<int32_t> end((size_t)n), pmax((size_t)n);
    int32_t part_max[LFQ_HOST_PARTS];
    bool part_sorted[LFQ_HOST_PARTS];
    int parts = 1;
    lfq_for_reads(n, [&](int64_t r0, int64_t r1, int part) {
        int32_t run = INT32_MIN;
        bool sorted = true;
        for (int64_t r = r0; r < r1; r++) {
            const uint32_t *cg = rs->cigar + rs->cigar_off[r];
            const int nc = (int)(rs->cigar_off[r + 1] - rs->cigar_off[r]);
            int64_t e = rs->pos[r];
            for (int k = 0; k < nc; k++) {
                const int op = cg[k] & 0xf;
                if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) {
                    e += cg[k] >> 4;
                }
            }
            end[(size_t)r] = (int32_t)std::min<int64_t>(e, INT32_MAX);
            run = std::max(run, end[(size_t)r]);
            pmax[(size_t)r] = run;
            sorted = sorted && (r == 0 || rs->pos[r] >= rs->pos[r - 1]);
        }
        part_max[part] = run;
        part_sorted[part] = sorted;
    }, &parts);
    for (int q = 0; q < parts && md != LFQ_NO_MAX_DEPTH; q++) {
        if (!part_sorted[q]) {
            rs->keep_rc = LFQ_ERR_INVALID;          /* the rule is defined on file order; bam_mplp_auto refuses such files */
            return rs->keep_rc;
        }
    }
    auto bed_only = [&]() {                         /* the mask is the BED's (none where it keeps every read) */
        if (bk && rs->n_bed_kept < n) {
            rs->keep = rs->bed_keep;
            rs->keep_end.swap(end);
            rs->n_kept = rs->n_bed_kept;
        }
        return LFQ_OK;
    };
    if (md == LFQ_NO_MAX_DEPTH) {
        return bed_only();
    }
    if (parts > 1) {
        int32_t before[LFQ_HOST_PARTS];
        before[0] = INT32_MIN;
        for (int q = 1; q < parts; q++) {
            before[q] = std::max(before[q - 1], part_max[q - 1]);
        }
        lfq_for_reads(n, [&](int64_t r0, int64_t r1, int part) {
            for (int64_t r = r0; r < r1 && pmax[(size_t)r] < before[part]; r++) {
                pmax[(size_t)r] = before[part];
            }
        });
    }
    /* 2. the proof: reads before the first one whose running maximum reaches P end before P */
    std::atomic<bool> drops{false};
    lfq_for_reads(n, [&](int64_t r0, int64_t r1, int) {
        for (int64_t r = r0; r < r1 && !drops.load(std::memory_order_relaxed); r++) {
            if (r > 0 && rs->pos[r] == rs->pos[r - 1]) {
                continue;                           /* not the first read of its run */
            }
            const int32_t P = rs->pos[r];
            int64_t r_end = r + 1;
            while (r_end < n && rs->pos[r_end] == P) {
                r_end++;
            }
            const int64_t lo = std::lower_bound(pmax.begin(), pmax.begin() + r, P) - pmax.begin();
            if (r_end - lo > md) {
                drops.store(true, std::memory_order_relaxed);
            }
        }
    });
    if (!drops.load()) {
        return bed_only();
    }
    /* 3. the walk */
    rs->keep.assign((size_t)n, 0);
    std::priority_queue<int32_t, std::vector<int32_t>, std::greater<int32_t>> live;   /* ends of the kept reads still counted */
    int64_t kept = 0, prev = -1;                    /* prev: the read pushed before this one */
    for (int64_t r = 0; r < n; r++) {
        if (bk && !bk[r]) {
            continue;
        }
        const int32_t P = rs->pos[r];
        const bool first = prev < 0 || P != rs->pos[prev];
        prev = r;
        if (first) {
            while (!live.empty() && live.top() < P) {
                live.pop();
            }
        }
        if (first || (int64_t)live.size() < md) {
            rs->keep[(size_t)r] = 1;
            live.push(end[(size_t)r]);
            kept++;
        }
    }
    rs->n_kept = kept;
    if (kept == n) {
        rs->keep.clear();                           /* (the bound of step 2 is not tight: nothing dropped after all) */
    } else {
        rs->keep_end.swap(end);                     /* the ends go to the device with the mask: one rule for them, here */
    }
    return LFQ_OK;
}

/* the kept reads on the device for the pileup kernels: the mask up, the compaction kernels on `st`, an event behind them for
 * the other pileup's stream.  -> *kept_idx (null: every read is kept, the kernels run as without a cap) */
static int readset_keep_device(lfq_ctx *c, lfq_readset *rs, hipStream_t st, const int32_t **kept_idx, const int32_t **kept_pos,
                               const int32_t **kept_pmax)
{
    *kept_idx = *kept_pos = *kept_pmax = nullptr;
    LFQ_TRY(readset_keep(c, rs));
    if (!readset_masked(c, rs) || rs->keep.empty()) {
        return LFQ_OK;
    }
    const int64_t n = rs->n;
    const int64_t o_idx = lfq_al(n), o_pos = o_idx + lfq_al(n * 4), o_pmax = o_pos + lfq_al(n * 4), o_scr = o_pmax + lfq_al(n * 4),
                  total = o_scr + lfq_keep_compact_scratch(n);
    if (!rs->keep_dev_valid || rs->keep_dev_for != c->plp_max_depth) {
        if (!rs->d_keep || rs->cap[LFQ_RSC_KEEP] < (size_t)total) {
            if (rs->d_keep) {
                rs_cache_give(c, LFQ_RSC_KEEP, rs->d_keep, rs->cap[LFQ_RSC_KEEP]);
                rs->d_keep = nullptr;
            }
            rs->d_keep = (uint8_t *)rs_cache_take(c, LFQ_RSC_KEEP, (size_t)total, &rs->cap[LFQ_RSC_KEEP]);
            if (!rs->d_keep) {
                return LFQ_ERR_NOMEM;
            }
        }
        if (!rs->ev_keep) {
            LFQ_TRY_HIP(hipEventCreateWithFlags(&rs->ev_keep, hipEventDisableTiming));
        }
        uint8_t *d = rs->d_keep;
        LFQ_TRY_HIP(hipMemcpyAsync(d, rs->keep.data(), (size_t)n, hipMemcpyHostToDevice, st));
        LFQ_TRY_HIP(hipMemcpyAsync(d + o_scr, rs->keep_end.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));   /* ends: scratch head */
        LFQ_TRY(lfq_launch_keep_compact(d, (const int32_t *)rs->d_pos, n, d + o_scr, (int32_t *)(d + o_idx), (int32_t *)(d + o_pos),
                                        (int32_t *)(d + o_pmax), st));
        LFQ_TRY_HIP(hipEventRecord(rs->ev_keep, st));
        rs->keep_dev_valid = true;
        rs->keep_dev_for = c->plp_max_depth;
    } else {
        LFQ_TRY_HIP(hipStreamWaitEvent(st, rs->ev_keep, 0));
    }
    *kept_idx = (const int32_t *)(rs->d_keep + o_idx);
    *kept_pos = (const int32_t *)(rs->d_keep + o_pos);
    *kept_pmax = (const int32_t *)(rs->d_keep + o_pmax);
    return LFQ_OK;
}

/* ---- the device view of the reads (LfqReadsDev, lfq_internal.h) ---------------------------------------------------------------
 * What every read-set step hands its kernels, filled here and nowhere else.  An array the read set does not have (yet) is null:
 * lb before lfq_readset_baq, the source-quality byte before lfq_readset_source_qual, BI / BD that neither the caller nor
 * lfq_readset_indelqual gave; after lfq_readset_indelqual every read has both tags, so no flags are consulted. */
static void readset_view(const lfq_readset *rs, LfqReadsDev *v)
{
    v->n_reads = rs->n;
    v->pos = (const int32_t *)rs->d_pos;
    v->cigar_off = (const int64_t *)rs->d_coff;
    v->seq_off = (const int64_t *)rs->d_soff;
    v->cigar = (const uint32_t *)rs->d_cig;
    v->seq = rs->d_seq;
    v->qual = rs->d_qual;
    v->mapq = rs->d_mapq;
    v->reverse = rs->d_rev;
    v->ref = rs->d_ref;
    v->ref_len = rs->ref_len;
    v->baq = rs->has_lb ? rs->d_lb : nullptr;
    v->sq = rs->has_sqb ? rs->d_sqb : nullptr;
    v->bi = rs->has_bi ? rs->d_bi : nullptr;
    v->bd = rs->has_bd ? rs->d_bd : nullptr;
    v->tag_flags = rs->idq_mode ? nullptr : rs->d_fl;
    v->pmax_end = nullptr;
    v->read_idx = nullptr;
}

/* ... for a pileup entry: sorted or refused (readset_pmax), then the -d cap -- the kernels walk the kept reads only, one decision
 * per read set and cap value, so that the column lists of the pileups agree.  Queues on `st` what readset_pmax and
 * readset_keep_device queue, in that order. */
static int readset_pileup_view(lfq_ctx *c, lfq_readset *rs, hipStream_t st, bool unsorted_may, LfqReadsDev *v)
{
    readset_view(rs, v);
    LFQ_TRY(readset_pmax(c, rs, st, unsorted_may));
    v->pmax_end = rs->d_pmax;
    const int32_t *k_idx, *k_pos, *k_pmax;
    LFQ_TRY(readset_keep_device(c, rs, st, &k_idx, &k_pos, &k_pmax));
    if (k_idx) {                            /* (null: cap and targets drop nothing, or there are none) */
        v->n_reads = rs->n_kept;
        v->read_idx = k_idx;
        v->pos = k_pos;
        v->pmax_end = rs->d_pmax ? k_pmax : nullptr;    /* (unsorted reads under targets alone: the read-major kernels, still) */
    }
    return LFQ_OK;
}

int lfq_readset_ref_from_device(const lfq_readset *rs) { return rs && rs->ref_from_device ? 1 : 0; }

int lfq_readset_kept_reads(lfq_ctx *c, lfq_readset *rs, uint8_t *keep_out, int64_t *n_kept_out)
{
    if (!c || !rs || rs->c != c) {
        return LFQ_ERR_INVALID;
    }
    LFQ_TRY(readset_keep(c, rs));
    const bool capped = readset_masked(c, rs);
    if (keep_out && rs->n > 0) {
        if (capped && !rs->keep.empty()) {
            memcpy(keep_out, rs->keep.data(), (size_t)rs->n);
        } else {
            memset(keep_out, 1, (size_t)rs->n);
        }
    }
    if (n_kept_out) {
        *n_kept_out = capped ? rs->n_kept : rs->n;
    }
    return LFQ_OK;
}

int lfq_readset_fetch_tags(lfq_ctx *c, lfq_readset *rs, uint8_t *lb_out, uint8_t *ai_out, uint8_t *ad_out, uint8_t *tag_flags)
{
    if (!c || !rs || rs->c != c) {
        return LFQ_ERR_INVALID;
    }
    if (rs->n == 0) {
        return LFQ_OK;
    }
    if ((lb_out && !rs->has_lb) || ((ai_out || ad_out || tag_flags) && !rs->has_idaq)) {
        return LFQ_ERR_INVALID;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(readset_upload_wait(rs));
    LFQ_TRY(readset_baq_wait(rs));
    if (lb_out) LFQ_TRY_HIP(hipMemcpyAsync(lb_out, rs->d_lb, (size_t)rs->n_bases, hipMemcpyDeviceToHost, c->stream));
    if (ai_out) LFQ_TRY_HIP(hipMemcpyAsync(ai_out, rs->d_ai, (size_t)rs->n_bases, hipMemcpyDeviceToHost, c->stream));
    if (ad_out) LFQ_TRY_HIP(hipMemcpyAsync(ad_out, rs->d_ad, (size_t)rs->n_bases, hipMemcpyDeviceToHost, c->stream));
    LFQ_TRY_HIP(hipStreamSynchronize(c->stream));
    if (tag_flags) {
        for (int64_t r = 0; r < rs->n; r++) {
            tag_flags[r] = (uint8_t)((rs->fl[(size_t)r] >> 2) & 3u);       /* bit 0: ai, bit 1: ad (lfq_baq_idaq_batch) */
        }
    }
    return LFQ_OK;
}

static int readset_from_baq_reads(lfq_ctx *c, const lfq_baq_reads *rd, lfq_readset **rs)
{
    lfq_pileup_reads pr;
    memset(&pr, 0, sizeof(pr));
    pr.n_reads = rd->n_reads;
    pr.pos = rd->pos; pr.cigar_off = rd->cigar_off; pr.cigar = rd->cigar; pr.seq_off = rd->seq_off;
    pr.seq = rd->seq; pr.qual = rd->qual; pr.ref = rd->ref; pr.ref_len = rd->ref_len;
    if (pr.n_reads > 0 && !pr.seq) {
        return LFQ_ERR_INVALID;
    }
    return readset_create(c, &pr, nullptr, rs, false, false);
}

int lfq_baq_batch(lfq_ctx *c, const lfq_baq_reads *rd, int baq_extended, uint8_t *lb_out)
{
    return lfq_baq_idaq_batch(c, rd, baq_extended, lb_out, nullptr, nullptr, nullptr);
}

int lfq_baq_idaq_batch(lfq_ctx *c, const lfq_baq_reads *rd, int baq_extended, uint8_t *lb_out, uint8_t *ai_out,
                       uint8_t *ad_out, uint8_t *tag_flags)
{
    const bool want_idaq = ai_out && ad_out && tag_flags;
    if (!c || !rd || rd->n_reads < 0 || (rd->n_reads > 0 && (!rd->pos || !rd->cigar_off || !rd->cigar || !rd->seq_off
                                                              || !rd->seq || !rd->qual || !rd->ref || !lb_out))) {
        return LFQ_ERR_INVALID;
    }
    if (rd->n_reads == 0) {
        return LFQ_OK;
    }
    lfq_readset *rs = nullptr;
    LFQ_TRY(readset_from_baq_reads(c, rd, &rs));
    int rc = lfq_readset_baq(c, rs, baq_extended, want_idaq ? 1 : 0);
    if (rc == LFQ_OK) {
        rc = lfq_readset_fetch_tags(c, rs, lb_out, want_idaq ? ai_out : nullptr, want_idaq ? ad_out : nullptr,
                                    want_idaq ? tag_flags : nullptr);
    }
    lfq_readset_destroy(rs);
    return rc;
}

/* bam_prob_realn_core_ext for every read of the set: lb (and ai / ad) stay on the device.  skip (lfq_readset_baq_fill; null: no
 * read is left out): skip[r] != 0 leaves read r out of every launch list -- its lb stays 0, its ai / ad '~', its tag flags clear.
 * merge (lfq_readset_baq_fill again): behind the HMM kernels, on their stream, the merge pass puts the stored bytes of the reads
 * and tags of rs->take in place of what is there.  No read left in: no HMM launch, and the context's BAQ times stay as they are.
 * stats: how many reads the launch lists held and how many launches took them. */
static int readset_baq_run(lfq_ctx *c, lfq_readset *rs, int baq_extended, bool want_idaq, const uint8_t *skip, bool merge,
                           lfq_baq_fill_stats *stats = nullptr)
{
    const lfq_readset *rd = rs;             /* the host views carry the names the geometry code below uses */
    const int64_t n = rs->n;
    if (n == 0) {
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(readset_baq_wait(rs));
    LFQ_TRY_HIP(hipStreamSynchronize(c->stream));   /* the pinned geometry / order buffers below may still be on their way out */
    double tmb[5] = {lfq_now_ms(), 0, 0, 0, 0};
    /* geometry of every read: alignment window and band width (bam_md_ext.c:312-380, :396-399) */
    /* (pinned, grow-only host buffers: 28 bytes per read are written once by the threads below and go out by DMA; a
     * std::vector would zero 56 MB for 2 M reads first and be copied through a staging buffer afterwards) */
    const int64_t h_bytes = lfq_al(n * (int64_t)sizeof(LfqBaqGeom)), ord_bytes = lfq_al(n * 4);
    LFQ_TRY(grow_pinned(&c->h_pin, &c->pin_bytes, h_bytes + ord_bytes));
    LfqBaqGeom *h = (LfqBaqGeom *)c->h_pin;
    int32_t *order = (int32_t *)(c->h_pin + h_bytes);
    /* (from the context's pinned pool: fresh memory would be page-faulted in by the threads below while the upload
     * thread is pinning the caller's arrays -- the two fight over the address-space lock) */
    LfqPin<int32_t> width(c, (size_t)n);
    LFQ_PIN_OK(width);
    const bool use_lds = lfq_knobs().baq_lds != 0;
    int max_lq = 0, max_w = 0;
    int part_lq[LFQ_HOST_PARTS] = {0}, part_w[LFQ_HOST_PARTS] = {0};
    int64_t part_narrow[LFQ_HOST_PARTS + 1] = {0}, part_band8[LFQ_HOST_PARTS + 1] = {0}, part_plain[LFQ_HOST_PARTS + 1] = {0};
    int64_t part_sel[LFQ_HOST_PARTS + 1] = {0};                     /* reads that are not skipped */
    LfqPin<uint8_t> has_id(c, (size_t)n);                            /* the read has an I or D operation (what idaq looks at) */
    LFQ_PIN_OK(has_id);
    int part_lrn[LFQ_HOST_PARTS] = {0}, part_lqn[LFQ_HOST_PARTS] = {0};
    int parts = 1;
    lfq_for_reads(n, [&](int64_t r_begin, int64_t r_end, int part) {
    int max_lq = 0, max_w = 0, lrn = 0, lqn = 0;    /* of this part */
    int64_t n_nar = 0, n_b8 = 0, n_pl = 0, n_in = 0;
    for (int64_t r = r_begin; r < r_end; r++) {
        LfqBaqGeom &o = h[(size_t)r];
        if (skip && skip[r]) {                          /* in no list: no launch reads its geometry */
            o.xb = o.l_ref = o.bw = 0;
            has_id[(size_t)r] = 0;
            width[(size_t)r] = -1;
            continue;
        }
        n_in++;
        const int l_qseq = (int)(rd->seq_off[r + 1] - rd->seq_off[r]);
        const uint32_t *cg = rd->cigar + rd->cigar_off[r];
        const int n_cigar = (int)(rd->cigar_off[r + 1] - rd->cigar_off[r]);
        int x = rd->pos[r], y = 0, yb = -1, ye = -1, xb = -1, xe = -1;
        bool indel_op = false;
        for (int k = 0; k < n_cigar; ++k) {
            const int op = cg[k] & 0xf, l = cg[k] >> 4;
            indel_op = indel_op || op == 1 || op == 2;
            if (op == 0 || op == 7 || op == 8) {
                if (yb < 0) yb = y;
                if (xb < 0) xb = x;
                ye = y + l; xe = x + l;
                x += l; y += l;
            } else if (op == 4 || op == 1) {
                y += l;
            } else if (op == 2 || op == 3) {
                x += l;
            }
        }
        has_id[(size_t)r] = indel_op ? 1 : 0;
        int bw = 7;
        if (abs((xe - xb) - (ye - yb)) > bw) bw = abs((xe - xb) - (ye - yb)) + 3;
        xb -= yb + bw / 2; if (xb < 0) xb = 0;
        xe += l_qseq - ye + bw / 2;
        if (xe - xb - l_qseq > bw) {
            xb += (xe - xb - l_qseq - bw) / 2, xe -= (xe - xb - l_qseq - bw) / 2;
        }
        if (xe > rd->ref_len) xe = (int)rd->ref_len;      /* the reference stops at the string's NUL */
        o.xb = xb;
        o.l_ref = xe - xb;
        o.bw = bw;
        int wr = 0;
        if (l_qseq > 0 && o.l_ref > 0) {
            int b2 = std::max(o.l_ref, l_qseq);
            if (b2 > bw) b2 = bw;
            if (b2 < abs(o.l_ref - l_qseq)) b2 = abs(o.l_ref - l_qseq);
            max_lq = std::max(max_lq, l_qseq);
            max_w = std::max(max_w, (b2 * 2 + 1) * 3 + 6);
            wr = (b2 * 2 + 1) * 3 + 6;
        }
        width[(size_t)r] = wr;
        /* narrow-band reads (rows of at most LFQ_BAQ_LDS_CELLS cells, a short reference window) run in the register kernel */
        if (use_lds && wr <= LFQ_BAQ_LDS_CELLS && o.l_ref <= LFQ_BAQ_LDS_MAX_LREF) {
            n_nar++;
            n_pl += (want_idaq && indel_op) ? 0 : 1;
            lrn = std::max(lrn, o.l_ref);
            lqn = std::max(lqn, l_qseq);
        } else if (use_lds && wr == LFQ_BAQ_BAND8_CELLS && o.l_ref <= LFQ_BAQ_LDS_MAX_LREF) {
            n_b8++;                                     /* band 8: a deletion of odd length (bam_md_ext.c:353-356) */
            lqn = std::max(lqn, l_qseq);
        }
    }
    part_lq[part] = max_lq;
    part_w[part] = max_w;
    part_narrow[part + 1] = n_nar;
    part_plain[part + 1] = n_pl;
    part_band8[part + 1] = n_b8;
    part_sel[part + 1] = n_in;
    part_lrn[part] = lrn;
    part_lqn[part] = lqn;
    }, &parts);
    int max_lref_narrow = 0, max_lq_narrow = 0;
    for (int p = 0; p < parts; p++) {
        max_lq = std::max(max_lq, part_lq[p]);
        max_w = std::max(max_w, part_w[p]);
        max_lref_narrow = std::max(max_lref_narrow, part_lrn[p]);
        max_lq_narrow = std::max(max_lq_narrow, part_lqn[p]);
        part_narrow[p + 1] += part_narrow[p];
        part_plain[p + 1] += part_plain[p];
        part_band8[p + 1] += part_band8[p];
        part_sel[p + 1] += part_sel[p];
    }
    const int64_t n_run = part_sel[parts];          /* the reads of the launch lists: all of them without `skip` */
    tmb[1] = lfq_now_ms();
    /* launch order: the narrow-band reads first, in input order (neighbouring reads share their reference window in the
     * caches), then the band-8 reads, the others behind them.  Every part of the read range knows where its reads go. */
    /* (with idaq the narrow-band reads without an I / D operation come first: for them the idaq instantiation does
     * nothing the plain one does not do -- ai / ad stay '~', no tag flag -- but runs 17 % longer) */
    const int64_t n_narrow = part_narrow[parts], n_band8 = part_band8[parts], n_plain = part_plain[parts];
    lfq_for_reads(n, [&](int64_t r_begin, int64_t r_end, int part) {
        int64_t pi = part_plain[part], ni = n_plain + (part_narrow[part] - part_plain[part]), bi = n_narrow + part_band8[part];
        int64_t wi = n_run - 1 - (part_sel[part] - part_narrow[part] - part_band8[part]);    /* wide reads before this part */
        for (int64_t r = r_begin; r < r_end; r++) {
            if (width[(size_t)r] < 0) {
                continue;                           /* skipped */
            }
            const bool short_ref = h[(size_t)r].l_ref <= LFQ_BAQ_LDS_MAX_LREF;
            if (use_lds && width[(size_t)r] <= LFQ_BAQ_LDS_CELLS && short_ref) {
                if (want_idaq && has_id[(size_t)r]) {
                    order[(size_t)ni++] = (int32_t)r;
                } else {
                    order[(size_t)pi++] = (int32_t)r;
                }
            } else if (use_lds && width[(size_t)r] == LFQ_BAQ_BAND8_CELLS && short_ref) {
                order[(size_t)bi++] = (int32_t)r;
            } else {
                order[(size_t)wi--] = (int32_t)r;
            }
        }
    });
    const int64_t n_bases = rs->n_bases;
    if (!rs->tag_blob) {                        /* lb (+ ai, ad): resident from here on */
        const int64_t each = lfq_al(n_bases + 16);
        rs->tag_blob = (uint8_t *)rs_cache_take(c, LFQ_RSC_TAGS, (size_t)(each * (want_idaq ? 3 : 1)), &rs->cap[LFQ_RSC_TAGS]);
        if (!rs->tag_blob) {
            return LFQ_ERR_NOMEM;
        }
        rs->d_lb = rs->tag_blob;
        rs->d_ai = want_idaq ? rs->tag_blob + each : nullptr;
        rs->d_ad = want_idaq ? rs->tag_blob + 2 * each : nullptr;
        LFQ_TRY_HIP(hipEventCreateWithFlags(&rs->ev_baq, hipEventDisableTiming));
        if (want_idaq) {
            rs->d_tagfl = (uint8_t *)rs_cache_take(c, LFQ_RSC_TAGFL, (size_t)n, &rs->cap[LFQ_RSC_TAGFL]);
            rs->h_fl_pin = (uint8_t *)rs_cache_take(c, LFQ_RSC_PINFL, (size_t)n, &rs->cap[LFQ_RSC_PINFL]);
            if (!rs->d_tagfl || !rs->h_fl_pin) {
                return LFQ_ERR_NOMEM;
            }
        }
    } else if (want_idaq && !rs->d_ai) {
        return LFQ_ERR_INVALID;                 /* a second BAQ pass that suddenly wants ai / ad: make a new read set */
    }
    /* the quality table outlives the call: the copy below is asynchronous and this function returns when it is queued */
    static const float *const h_q2p = [] {
        static float t[256];
        for (int i = 0; i < 256; i++) {
            t[i] = (float)pow(10, -i / 10.);                 /* kprobaln_ext.c:121-123 */
        }
        return (const float *)t;
    }();
    /* per-call device data: geometry, launch order, the quality table (the reads themselves are resident) */
    uint8_t *d_blob = nullptr;
    const int64_t o_reads = 0, o_q2p = o_reads + lfq_al(n * (int64_t)sizeof(LfqBaqGeom)), o_ord = o_q2p + lfq_al(1024),
                  total = o_ord + lfq_al(n * 4);
    LFQ_TRY(grow(&c->d_tmp[0], &c->tmp_bytes[0], total));
    d_blob = c->d_tmp[0];
    int rc = LFQ_OK;
    auto up = [&](int64_t off, const void *src, int64_t bytes) {
        if (rc == LFQ_OK && bytes > 0 && hipMemcpyAsync(d_blob + off, src, (size_t)bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            rc = LFQ_ERR_HIP;
        }
    };
    up(o_reads, h, n * (int64_t)sizeof(LfqBaqGeom));
    up(o_q2p, h_q2p, 1024);
    up(o_ord, order, n * 4);
    if (rc == LFQ_OK && (hipMemsetAsync(rs->d_lb, 0, (size_t)std::max<int64_t>(n_bases, 1), c->stream) != hipSuccess
                         || (want_idaq && (hipMemsetAsync(rs->d_ai, '~', (size_t)n_bases, c->stream) != hipSuccess
                                           || hipMemsetAsync(rs->d_ad, '~', (size_t)n_bases, c->stream) != hipSuccess
                                           || hipMemsetAsync(rs->d_tagfl, 0, (size_t)n, c->stream) != hipSuccess)))) {
        rc = LFQ_ERR_HIP;
    }
    tmb[2] = lfq_now_ms();
    double *d_scr = nullptr;
    int32_t *d_expect = nullptr;
    uint8_t *d_tmp8 = nullptr;
    if (rc == LFQ_OK && max_lq > 0) {
        LfqBaqArgs A;
        memset(&A, 0, sizeof(A));
        readset_view(rs, &A);
        A.geom = (const LfqBaqGeom *)(d_blob + o_reads);
        A.lb_out = rs->d_lb;
        A.qual2prob = (const float *)(d_blob + o_q2p);
        A.rows = max_lq + 1;
        A.W = max_w;
        A.baq_extended = baq_extended ? 1 : 0;
        A.par_d = c->baq_par_d;
        A.par_e = c->baq_par_e;
        /* waves per launch from a 4 GiB scratch budget */
        const int64_t per_wave = ((int64_t)A.rows * A.W + 2 * (int64_t)A.W + 2 * ((int64_t)A.rows + 2)) * 64 * 8;
        /* the kernel is a chain of dependent HBM accesses per lane: it needs several wavefronts per SIMD in
         * flight, i.e. scratch for them -- up to half of the free HBM, at most 32 GiB */
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        int64_t budget_b = std::min<int64_t>((int64_t)32 << 30, (int64_t)(free_b / 2));
        if (lfq_knobs().baq_scratch_mb >= 0) {
            budget_b = (int64_t)lfq_knobs().baq_scratch_mb << 20;
        }
        /* + 3: the four groups of reads (plain narrow, narrow with indels, band 8, wide) round up to whole wavefronts separately */
        int64_t waves = std::max<int64_t>(1, std::min<int64_t>((n_run + 63) / 64 + 3, budget_b / per_wave));
        auto keep = [&](auto **slot, int64_t *have, int64_t need) {
            if (need > *have) {
                if (*slot) (void)hipFree(*slot);
                *slot = nullptr;
                *have = 0;
                if (hipMalloc((void **)slot, (size_t)need) != hipSuccess) {
                    rc = LFQ_ERR_NOMEM;
                    return;
                }
                *have = need;
            }
        };
        keep(&c->d_baq_scr, &c->baq_scr_bytes, waves * per_wave);
        /* several contexts of one process (a host thread each) size their scratch from the same "free" figure at the same time: a
         * context that comes too late for its share takes fewer wavefronts per launch instead of failing -- down to one round of the
         * SIMDs, below which the kernel would leave part of the device idle */
        while (rc == LFQ_ERR_NOMEM && waves > (int64_t)c->n_cu * 4) {
            (void)hipGetLastError();
            rc = LFQ_OK;
            waves = std::max<int64_t>((int64_t)c->n_cu * 4, waves / 2);
            keep(&c->d_baq_scr, &c->baq_scr_bytes, waves * per_wave);
        }
        if (rc == LFQ_OK && c->baq_scr_bytes / per_wave < waves) {
            waves = c->baq_scr_bytes / per_wave;
        }
        keep(&c->d_baq_expect, &c->baq_expect_bytes, waves * A.rows * 64 * 4);
        keep(&c->d_baq_tmp8, &c->baq_tmp8_bytes, waves * 2 * A.rows * 64);
        if (!lfq_knobs().baq_one_variant) {
            keep(&c->d_baq_nflag, &c->baq_nflag_bytes, (n + 63) / 64 + 64);
        }
        if (want_idaq) {
            keep(&c->d_baq_itab, &c->baq_itab_bytes, waves * LFQ_BAQ_MAX_INDELS * 4 * 64 * 4);
            keep(&c->d_baq_terms, &c->baq_terms_bytes, waves * (int64_t)LFQ_BAQ_MAX_TERMS * 64 * 8);
            A.itab = c->d_baq_itab;
            A.terms = c->d_baq_terms;
            A.ai_out = rs->d_ai;
            A.ad_out = rs->d_ad;
            A.tagfl_out = rs->d_tagfl;
        }
        d_scr = c->d_baq_scr;
        d_expect = c->d_baq_expect;
        d_tmp8 = c->d_baq_tmp8;
        A.scratch = d_scr;
        A.expect = d_expect;
        A.tmp8 = d_tmp8;
        A.order = (const int32_t *)(d_blob + o_ord);
        A.max_lref = max_lref_narrow;
        A.lds_rows = max_lq_narrow + 1;
        /* The reads with a wider band are few: band 8 (a deletion of odd length; the register kernel's second
         * instantiation) and everything beyond (the all-HBM kernel, a handful of latency-bound wavefronts).  They run
         * beside the narrow-band launches on the side streams, in scratch slots of their own behind the narrow ones'
         * (wavefront w of a launch owns slot w).  The narrow-band kernel runs one wavefront per SIMD, so a launch is cut
         * to a whole number of rounds over the SIMDs: a launch of 7.3 rounds takes as long as one of 8. */
        const int64_t n_wide = n_run - n_narrow - n_band8;
        const int64_t waves_wide = (n_wide + 63) / 64, waves_b8 = (n_band8 + 63) / 64;
        const bool side_ok = n_narrow > 0 && c->side[0] != nullptr && c->side[1] != nullptr && !lfq_knobs().single_stream;
        const bool beside = side_ok && waves_wide + waves_b8 > 0 && waves_wide + waves_b8 < waves / 4;
        /* (The narrow-band reads with an indel operation -- the IDAQ instantiation: 4 % of the bench's reads -- stay behind the
         * plain launches on c->stream: beside them a lone BAQ + IDAQ call went 6.2 -> 5.3 ms per 400 K reads, the reads -> VCF
         * chain 37.7 -> 39.0 ms per region.) */
        const bool use_side0 = beside && n_wide > 0, use_side1 = beside && n_band8 > 0;
        int64_t waves_n = waves - (beside ? waves_wide + waves_b8 : 0);      /* slots of a narrow launch */
        const int64_t round = (int64_t)c->n_cu * 4;
        if ((n_narrow + 63) / 64 > waves_n && waves_n > round) {       /* more than one launch: whole rounds each */
            waves_n = waves_n / round * round;
        }
        auto at_slot = [&](int64_t slot) {          /* the arguments with the scratch of wavefront slot `slot` first */
            LfqBaqArgs X = A;
            X.scratch = A.scratch + (size_t)slot * (size_t)(per_wave / 8);
            X.expect = A.expect + (size_t)slot * A.rows * 64;
            X.tmp8 = A.tmp8 + (size_t)slot * 2 * A.rows * 64;
            if (want_idaq) {
                X.itab = A.itab + (size_t)slot * LFQ_BAQ_MAX_INDELS * 4 * 64;
                X.terms = A.terms + (size_t)slot * LFQ_BAQ_MAX_TERMS * 64;
            }
            return X;
        };
        /* The reads may still be crossing PCIe (lfq_readset_create): a launch waits for the chunks of bases and qualities
         * that hold its reads -- the plain narrow-band launches walk the reads in input order, so the first one starts
         * after a quarter of them --, everything else for all of them. */
        if ((use_side0 || use_side1) && hipEventRecord(c->ev_join[0], c->stream) != hipSuccess) {
            rc = LFQ_ERR_HIP;       /* the side streams start after the uploads / memsets queued on c->stream so far */
        }
        if (rc == LFQ_OK) {
            rc = c->baq_t.begin(c->stream);     /* around the call's BAQ kernels (lfq_last_baq_times) */
        }
        c->baq_launches = 0;
        c->baq_reads = n_run;
        c->baq_bases = n_bases;
        {
            LfqBaqArgs Ap = A;                      /* the plain instantiation: no indel table */
            Ap.itab = nullptr;
            Ap.terms = nullptr;
            Ap.ai_out = Ap.ad_out = nullptr;
            Ap.tagfl_out = nullptr;
            /* (while the reads are still arriving the first launch takes one round only: it starts when the small first
             * chunk of lfq_readset_create has landed, and the link stays ahead of the kernel from there on) */
            const bool early = (rs->up_thread || rs->up_events) && rs->up_nchunks == LFQ_UP_CHUNKS && waves_n >= 4 * round
                               && n_plain > 16 * round * 64;
            int64_t ramp = early ? round : waves_n;             /* wavefronts of the next launch: 1, 2, 4 rounds, then all slots */
            std::vector<std::pair<LfqBaqArgs, int64_t>> with_n;
            for (int64_t first = 0, cnt = 0; rc == LFQ_OK && first < n_plain; first += cnt) {
                cnt = std::min<int64_t>(std::min(ramp, waves_n) * 64, n_plain - first);
                ramp = ramp < 4 * round ? ramp * 2 : waves_n;
                rc = readset_upload_wait_reads(rs, order[(size_t)(first + cnt - 1)], c->stream);
                Ap.first_read = (int32_t)first;
                /* (first is a multiple of 64: the launches are cut to whole wavefronts) */
                Ap.nflag = (c->d_baq_nflag && !lfq_knobs().baq_one_variant) ? c->d_baq_nflag + first / 64 : nullptr;
                if (rc == LFQ_OK) {
                    rc = lfq_launch_baq(Ap, cnt, 1, c->stream, Ap.nflag ? 1 : 0);
                    c->baq_launches++;
                    if (Ap.nflag) {
                        with_n.push_back({Ap, cnt});
                    }
                }
            }
            /* The instantiation with the N case for every launch's flagged wavefronts, behind all of them: a wavefront of
             * this kernel needs an empty SIMD even to find that it has nothing to do, and a launch that came up while the
             * indel counter pass of the chain kept every SIMD busy waited for that kernel to drain (1.2 ms per region for
             * wavefronts that leave at once).  Here the other streams are idle or done; the scratch slots of a launch's
             * wavefronts are free again (every earlier launch has finished: stream order). */
            for (const auto &w : with_n) {
                if (rc == LFQ_OK) {
                    rc = lfq_launch_baq(w.first, w.second, 1, c->stream, 2);
                }
            }
        }
        if (rc == LFQ_OK) {
            rc = readset_upload_wait_inputs(rs, {c->stream, c->side[0], c->side[1]});
        }
        if (use_side0 || use_side1) {
            /* wide-band and band-8 reads on the side streams, beside the plain narrow-band launches; c->stream ends after them */
            if (rc == LFQ_OK && use_side0 && hipStreamWaitEvent(c->side[0], c->ev_join[0], 0) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
            if (rc == LFQ_OK && beside && n_wide > 0) {
                LfqBaqArgs Aw = at_slot(waves_n + waves_b8);
                Aw.first_read = (int32_t)(n_narrow + n_band8);
                rc = lfq_launch_baq(Aw, n_wide, 0, c->side[0]);
            }
            if (rc == LFQ_OK && use_side1 && hipStreamWaitEvent(c->side[1], c->ev_join[0], 0) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
            if (rc == LFQ_OK && beside && n_band8 > 0) {
                LfqBaqArgs Ab = at_slot(waves_n);
                Ab.first_read = (int32_t)n_narrow;
                rc = lfq_launch_baq(Ab, n_band8, 2, c->side[1]);
            }
            if (rc == LFQ_OK && ((use_side0 && hipEventRecord(c->ev_join[1], c->side[0]) != hipSuccess)
                                 || (use_side1 && hipEventRecord(c->ev_join[2], c->side[1]) != hipSuccess))) {
                rc = LFQ_ERR_HIP;
            }
        }
        for (int64_t first = n_plain; rc == LFQ_OK && first < n_narrow; first += waves_n * 64) {
            A.first_read = (int32_t)first;
            rc = lfq_launch_baq(A, std::min<int64_t>(waves_n * 64, n_narrow - first), 1, c->stream);
            c->baq_launches++;
        }
        if (rc == LFQ_OK && ((use_side0 && hipStreamWaitEvent(c->stream, c->ev_join[1], 0) != hipSuccess)
                             || (use_side1 && hipStreamWaitEvent(c->stream, c->ev_join[2], 0) != hipSuccess))) {
            rc = LFQ_ERR_HIP;
        }
        if (!beside) {
            for (int64_t first = n_narrow; rc == LFQ_OK && first < n_narrow + n_band8; first += waves * 64) {
                A.first_read = (int32_t)first;
                rc = lfq_launch_baq(A, std::min<int64_t>(waves * 64, n_narrow + n_band8 - first), 2, c->stream);
                c->baq_launches++;
            }
            for (int64_t first = n_narrow + n_band8; rc == LFQ_OK && first < n_run; first += waves * 64) {
                A.first_read = (int32_t)first;
                rc = lfq_launch_baq(A, std::min<int64_t>(waves * 64, n_run - first), 0, c->stream);
                c->baq_launches++;
            }
        }
    }
    if (rc == LFQ_OK && !(skip && n_run == 0)) {
        rc = c->baq_t.end(c->stream);
    }
    tmb[3] = lfq_now_ms();
    if (rc == LFQ_OK && merge) {
        /* the stored tags over the computed ones, and their ai / ad bits into what the flag merge below reads */
        uint8_t *const dst[3] = {rs->d_lb, want_idaq ? rs->d_ai : nullptr, want_idaq ? rs->d_ad : nullptr};
        if (hipMemcpyAsync(rs->d_take, rs->take.data(), (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            rc = LFQ_ERR_HIP;
        }
        if (rc == LFQ_OK) {
            rc = c->fill_t.begin(c->stream);
        }
        if (rc == LFQ_OK) {
            rc = lfq_bam_merge((const int64_t *)rs->d_soff, rs->d_take, rs->d_st, dst, want_idaq ? rs->d_tagfl : nullptr, n, n_bases,
                               c->stream);
        }
        if (rc == LFQ_OK) {
            rc = c->fill_t.end(c->stream);
        }
    }
    /* which reads got an ai / ad tag (bam_md_ext.c:238-243) joins the resident flags as bits 2, 3 on the device; the
     * merged byte travels to pinned memory for the host's event tables.  Nothing here waits for the kernels. */
    if (rc == LFQ_OK && want_idaq) {
        rc = lfq_launch_flag_merge(rs->d_fl, rs->d_tagfl, n, c->stream);
        if (rc == LFQ_OK && hipMemcpyAsync(rs->h_fl_pin, rs->d_fl, (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
            rc = LFQ_ERR_HIP;
        }
    }
    if (rc == LFQ_OK && hipEventRecord(rs->ev_baq, c->stream) != hipSuccess) {
        rc = LFQ_ERR_HIP;
    }
    if (rc != LFQ_OK) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    rs->baq_pending = true;
    rs->baq_idaq = want_idaq;
    tmb[4] = lfq_now_ms();
    if (lfq_timing_on) {
        (void)hipStreamSynchronize(c->stream);
        fprintf(stderr, "[lfq timing] baq: geometry %.1f  order + allocations + uploads %.1f  scratch + launches %.1f  kernels (sync, timing only) %.1f ms\n",
                tmb[1] - tmb[0], tmb[2] - tmb[1], tmb[3] - tmb[2], lfq_now_ms() - tmb[3]);
    }
    rs->has_lb = true;
    rs->filled = merge;
    if (want_idaq) {
        rs->has_idaq = true;
        rs->h_ai = rs->h_ad = nullptr;          /* superseded by the device result */
    }
    if (stats) {
        stats->n_need_hmm = n_run;
        stats->n_hmm_launches = n_run > 0 && max_lq > 0 ? c->baq_launches : 0;
    }
    return rc;
}

int lfq_readset_baq(lfq_ctx *c, lfq_readset *rs, int baq_extended, int want_idaq)
{
    if (!c || !rs || rs->c != c || (rs->n > 0 && !rs->qual)) {
        return LFQ_ERR_INVALID;
    }
    const bool want = want_idaq != 0;
    if (rs->bed && rs->n > 0) {
        /* plp.c:625-629 comes before the realignment: the HMM runs for the reads the targets keep */
        LFQ_TRY(readset_bed_keep(c, rs));
        std::vector<uint8_t> skip((size_t)rs->n);
        for (int64_t r = 0; r < rs->n; r++) {
            skip[(size_t)r] = rs->bed_keep[(size_t)r] ? 0 : 1;
        }
        if (rs->n_bed_kept == 0) {
            c->baq_launches = 0;                /* (no launch: readset_baq_run leaves the context's figures alone then) */
            c->baq_reads = 0;
            c->baq_bases = rs->n_bases;
        }
        return readset_baq_run(c, rs, baq_extended, want, skip.data(), false);
    }
    return readset_baq_run(c, rs, baq_extended, want, nullptr, false);
}

/* lfq_readset_baq where a tag is missing (include/lofreq_amd.h has the rule): need_r on the host, from the CIGARs and the stored
 * bits of the decode's aux pass */
int lfq_readset_baq_fill(lfq_ctx *c, lfq_readset *rs, int baq_extended, int want_idaq_i, int redo_baq)
{
    if (!c || !rs || rs->c != c || (rs->n > 0 && !rs->qual)) {
        return LFQ_ERR_INVALID;
    }
    const bool want_idaq = want_idaq_i != 0;
    const int64_t n = rs->n;
    lfq_baq_fill_stats &F = c->fill_stats;
    memset(&F, 0, sizeof(F));
    F.n_reads = n;
    c->fill_hmm = c->fill_merge = 0;
    const uint8_t *bk = nullptr;                        /* targets: the reads they drop need no tag at all */
    if (rs->bed && n > 0) {
        LFQ_TRY(readset_bed_keep(c, rs));
        bk = rs->bed_keep.data();
    }
    if (rs->stored_fl.empty() || n == 0) {
        std::vector<uint8_t> bed_skip;
        for (int64_t r = 0; bk && r < n; r++) {
            bed_skip.push_back(bk[r] ? 0 : 1);
        }
        const int rc = readset_baq_run(c, rs, baq_extended, want_idaq, bk ? bed_skip.data() : nullptr, false, &F);
        c->fill_hmm = rc == LFQ_OK && F.n_hmm_launches > 0;
        return rc;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(readset_baq_wait(rs));
    LFQ_TRY_HIP(hipStreamSynchronize(c->stream));       /* an earlier fill's copy of rs->take has left the host */
    const uint8_t keep_bits = (uint8_t)((redo_baq ? 0u : 1u) | (want_idaq ? 6u : 0u));
    rs->take.resize((size_t)n);
    std::vector<uint8_t> skip((size_t)n);
    int64_t part_cnt[LFQ_HOST_PARTS][3];
    int parts = 1;
    lfq_for_reads(n, [&](int64_t r0, int64_t r1, int part) {
        int64_t cnt[3] = {0, 0, 0};
        for (int64_t r = r0; r < r1; r++) {
            bool has_ins = false, has_del = false;
            for (int64_t k = rs->cigar_off[r]; k < rs->cigar_off[r + 1]; k++) {
                const uint32_t op = rs->cigar[k] & 0xf;
                has_ins = has_ins || op == 1;
                has_del = has_del || op == 2;
            }
            const uint8_t S = (bk && !bk[r]) ? (uint8_t)0 : (uint8_t)(rs->stored_fl[(size_t)r] & keep_bits);
            const bool need = (bk && !bk[r]) ? false : !(S & 1u) || (want_idaq && ((has_del && !(S & 4u)) || (has_ins && !(S & 2u))));
            skip[(size_t)r] = need ? 0 : 1;
            rs->take[(size_t)r] = S;
            for (int t = 0; t < 3; t++) {
                cnt[t] += (S >> t) & 1u;
            }
        }
        for (int t = 0; t < 3; t++) {
            part_cnt[part][t] = cnt[t];
        }
    }, &parts);
    const int rc = readset_baq_run(c, rs, baq_extended, want_idaq, skip.data(), true, &F);
    for (int q = 0; q < parts; q++) {
        F.n_stored_lb += part_cnt[q][0];
        F.n_stored_ai += part_cnt[q][1];
        F.n_stored_ad += part_cnt[q][2];
    }
    c->fill_hmm = rc == LFQ_OK && F.n_hmm_launches > 0;
    c->fill_merge = rc == LFQ_OK;
    return rc;
}

int lfq_last_baq_fill_stats(lfq_ctx *c, lfq_baq_fill_stats *s)
{
    if (!c || !s) {
        return LFQ_ERR_INVALID;
    }
    *s = c->fill_stats;
    s->ms_hmm = s->ms_merge = 0.f;
    if (c->fill_hmm || c->fill_merge) {
        LFQ_TRY_HIP(hipSetDevice(c->device));
    }
    if (c->fill_hmm) {
        LFQ_TRY(c->baq_t.ms(&s->ms_hmm));
    }
    if (c->fill_merge) {
        LFQ_TRY(c->fill_t.ms(&s->ms_merge));
    }
    return LFQ_OK;
}

int lfq_last_baq_times(lfq_ctx *c, lfq_baq_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    memset(t, 0, sizeof(*t));
    if (!c->baq_t.ev[1]) {
        return LFQ_OK;                  /* no BAQ call on this context yet */
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(c->baq_t.ms(&t->ms_kernels));
    t->n_launches = c->baq_launches;
    t->n_reads = c->baq_reads;
    t->n_bases = c->baq_bases;
    return LFQ_OK;
}

/* `lofreq indelqual` on the resident reads (kernels: lfq_indelqual.hip) */
int lfq_readset_indelqual(lfq_ctx *c, lfq_readset *rs, const lfq_indelqual_conf *conf)
{
    if (!c || !rs || rs->c != c || !conf || (conf->mode != LFQ_IDQ_UNIFORM && conf->mode != LFQ_IDQ_DINDEL)) {
        return LFQ_ERR_INVALID;
    }
    const int64_t n = rs->n, nb = rs->n_bases;
    const bool dindel = conf->mode == LFQ_IDQ_DINDEL;
    int64_t lo = INT64_MAX, hi = 0;         /* reference positions the M / = / X operations of the batch cover */
    if (dindel && n > 0) {
        /* what the reference cannot do (see the header), and the span of the table */
        int64_t part_lo[LFQ_HOST_PARTS], part_hi[LFQ_HOST_PARTS];
        bool part_bad[LFQ_HOST_PARTS];
        int parts = 1;
        lfq_for_reads(n, [&](int64_t r0, int64_t r1, int part) {
            int64_t plo = INT64_MAX, phi = 0;
            bool bad = false;
            for (int64_t r = r0; r < r1; r++) {
                int64_t x = rs->pos[r], y = 0;
                bad = bad || x < 0;
                for (int64_t k = rs->cigar_off[r]; k < rs->cigar_off[r + 1]; k++) {
                    const int op = (int)(rs->cigar[k] & 0xf);
                    const int64_t len = rs->cigar[k] >> 4;
                    if (op == 0 || op == 7 || op == 8) {
                        if (len > 0) {
                            plo = std::min(plo, x);
                            phi = std::max(phi, x + len);
                        }
                        x += len;
                        y += len;
                    } else if (op == 1 || op == 4) {
                        y += len;
                    } else if (op == 2) {
                        x += len;
                    } else if (op != 5) {
                        bad = true;                 /* "unknown op" (lofreq_indelqual.c:195) */
                    }
                }
                bad = bad || y != rs->seq_off[r + 1] - rs->seq_off[r];
            }
            part_lo[part] = plo;
            part_hi[part] = phi;
            part_bad[part] = bad;
        }, &parts);
        for (int q = 0; q < parts; q++) {
            if (part_bad[q]) {
                return LFQ_ERR_INVALID;
            }
            lo = std::min(lo, part_lo[q]);
            hi = std::max(hi, part_hi[q]);
        }
    }
    c->idq_times.ms_kernels = 0.f;
    c->idq_times.n_launches = 0;
    c->idq_times.n_reads = n;
    c->idq_times.n_bases = nb;
    if (n == 0 || nb == 0) {
        rs->idq_mode = 0;
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    /* Nothing here reads what lfq_readset_baq writes: beside a BAQ step that is still running the kernels take the stream the
     * indel pileup will take (see lfq_readset_pileup_indels); the event orders any other consumer behind them */
    hipStream_t qs = (rs->baq_pending && c->dps && !lfq_knobs().single_stream) ? c->dps : c->stream;
    const int64_t tab_begin = lo < hi ? lo / 16 * 16 : 0, tab_end = lo < hi ? std::min(hi, rs->ref_len) : 0;
    const int64_t each = lfq_al(nb + 16), o_tab = (dindel ? 1 : 2) * each;
    const int64_t total = o_tab + (dindel ? lfq_al(std::max<int64_t>(tab_end - tab_begin, 0) + 16) : 0);
    if (rs->ev_idq) {
        LFQ_TRY_HIP(hipEventSynchronize(rs->ev_idq));       /* a second pass over the same read set: the first one's kernels are done */
    } else {
        LFQ_TRY_HIP(hipEventCreateWithFlags(&rs->ev_idq, hipEventDisableTiming));
    }
    if (!rs->idq_blob || rs->cap[LFQ_RSC_IDQ] < (size_t)total) {
        rs_cache_give(c, LFQ_RSC_IDQ, rs->idq_blob, rs->cap[LFQ_RSC_IDQ]);
        rs->idq_blob = (uint8_t *)rs_cache_take(c, LFQ_RSC_IDQ, (size_t)total, &rs->cap[LFQ_RSC_IDQ]);
        if (!rs->idq_blob) {
            return LFQ_ERR_NOMEM;
        }
    }
    LfqIdqArgs A;
    memset(&A, 0, sizeof(A));
    readset_view(rs, &A);                                   /* (the uniform fill reads none of it) */
    A.n_bases = nb;
    A.bi_out = rs->idq_blob;
    A.bd_out = dindel ? rs->idq_blob : rs->idq_blob + each;
    int rc = LFQ_OK;
    if (dindel) {
        rc = readset_upload_wait_inputs(rs, {qs});          /* positions, CIGARs, offsets and the contig are on the device */
        A.tab = rs->idq_blob + o_tab;
        A.tab_begin = tab_begin;
        A.tab_end = tab_end;
    } else {
        auto encode_q = [](int64_t q) { return (uint8_t)(q < 33 ? '!' : (q > 126 ? '~' : q)); };   /* ENCODE_Q, :66 */
        rs->idq_ins = encode_q((int64_t)conf->ins_qual + 33);
        rs->idq_del = encode_q((int64_t)conf->del_qual + 33);
        A.ins_byte = rs->idq_ins;
        A.del_byte = rs->idq_del;
    }
    if (rc == LFQ_OK) {
        rc = c->idq_t.begin(qs);
    }
    if (rc == LFQ_OK && dindel && tab_end > tab_begin) {
        rc = lfq_launch_idq_table(rs->d_ref, rs->ref_len, tab_begin, tab_end, rs->idq_blob + o_tab, qs);
        c->idq_times.n_launches++;
    }
    if (rc == LFQ_OK) {
        rc = lfq_launch_idq_fill(A, qs);
        c->idq_times.n_launches++;
    }
    if (rc == LFQ_OK && (c->idq_t.end(qs) != LFQ_OK || hipEventRecord(rs->ev_idq, qs) != hipSuccess)) {
        rc = LFQ_ERR_HIP;
    }
    if (rc != LFQ_OK) {
        (void)hipStreamSynchronize(qs);
        return rc;
    }
    rs->idq_mode = conf->mode;
    rs->d_bi = A.bi_out;
    rs->d_bd = A.bd_out;
    rs->has_bi = rs->has_bd = true;
    rs->h_bi = rs->h_bd = nullptr;              /* superseded by the device result */
    return LFQ_OK;
}

int lfq_readset_fetch_indelquals(lfq_ctx *c, lfq_readset *rs, uint8_t *bi_out, uint8_t *bd_out)
{
    if (!c || !rs || rs->c != c) {
        return LFQ_ERR_INVALID;
    }
    if (rs->n == 0 || rs->n_bases == 0) {
        return LFQ_OK;
    }
    if (!rs->idq_mode) {
        return LFQ_ERR_INVALID;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY_HIP(hipStreamWaitEvent(c->stream, rs->ev_idq, 0));
    if (bi_out) LFQ_TRY_HIP(hipMemcpyAsync(bi_out, rs->d_bi, (size_t)rs->n_bases, hipMemcpyDeviceToHost, c->stream));
    if (bd_out) LFQ_TRY_HIP(hipMemcpyAsync(bd_out, rs->d_bd, (size_t)rs->n_bases, hipMemcpyDeviceToHost, c->stream));
    LFQ_TRY_HIP(hipStreamSynchronize(c->stream));
    return LFQ_OK;
}

int lfq_indelqual_batch(lfq_ctx *c, const lfq_baq_reads *rd, const lfq_indelqual_conf *conf, uint8_t *bi_out, uint8_t *bd_out)
{
    if (!c || !rd || !conf || rd->n_reads < 0 || (conf->mode != LFQ_IDQ_UNIFORM && conf->mode != LFQ_IDQ_DINDEL)
        || (rd->n_reads > 0 && (!rd->pos || !rd->cigar_off || !rd->cigar || !rd->seq_off || !rd->ref || !bi_out || !bd_out))) {
        return LFQ_ERR_INVALID;
    }
    if (rd->n_reads == 0) {
        memset(&c->idq_times, 0, sizeof(c->idq_times));
        return LFQ_OK;
    }
    /* the read set of this step holds what its kernels read: positions, CIGARs, offsets, the contig -- no bases, no qualities */
    lfq_pileup_reads pr;
    memset(&pr, 0, sizeof(pr));
    pr.n_reads = rd->n_reads;
    pr.pos = rd->pos; pr.cigar_off = rd->cigar_off; pr.cigar = rd->cigar; pr.seq_off = rd->seq_off;
    pr.ref = rd->ref; pr.ref_len = rd->ref_len;
    lfq_readset *rs = nullptr;
    LFQ_TRY(readset_create(c, &pr, nullptr, &rs, false, false));
    int rc = lfq_readset_indelqual(c, rs, conf);
    if (rc == LFQ_OK) {
        rc = lfq_readset_fetch_indelquals(c, rs, bi_out, bd_out);
    }
    lfq_readset_destroy(rs);
    return rc;
}

int lfq_last_indelqual_times(lfq_ctx *c, lfq_indelqual_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = c->idq_times;
    if (t->n_launches > 0) {
        LFQ_TRY_HIP(hipSetDevice(c->device));
        LFQ_TRY(c->idq_t.ms(&t->ms_kernels));
    }
    return LFQ_OK;
}

int lfq_pileup_snv_tracks(lfq_ctx *c, const lfq_pileup_reads *rd, int64_t region_begin, int64_t region_end,
                          int min_plp_bq, lfq_tracks *out, int64_t *col_pos_out)
{
    if (!c || !rd || !out || region_end < region_begin || rd->n_reads < 0
        || (rd->n_reads > 0 && (!rd->pos || !rd->cigar_off || !rd->cigar || !rd->seq_off || !rd->seq || !rd->qual
                                || !rd->mapq || !rd->reverse || !rd->ref))) {
        return LFQ_ERR_INVALID;
    }
    lfq_readset *rs = nullptr;
    LFQ_TRY(lfq_readset_create(c, rd, nullptr, &rs));
    const int rc = lfq_readset_pileup_snv(c, rs, region_begin, region_end, min_plp_bq, out, col_pos_out);
    lfq_readset_destroy(rs);            /* the tracks live in the context, not in the read set; waits for the scatter pass */
    return rc;
}

int lfq_readset_pileup_snv(lfq_ctx *c, lfq_readset *rs, int64_t region_begin, int64_t region_end, int min_plp_bq,
                           lfq_tracks *out, int64_t *col_pos_out)
{
    if (!c || !rs || rs->c != c || !out || region_end < region_begin
        || (rs->n > 0 && (!rs->qual || !rs->mapq || !rs->reverse))) {
        return LFQ_ERR_INVALID;
    }
    memset(out, 0, sizeof(*out));
    const int64_t n = rs->n, width = region_end - region_begin;
    if (n == 0 || width == 0) {
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(readset_upload_wait(rs, c->stream));
    /* per-position counters (kept until the next call) */
    const int64_t n_tiles = (width + LFQ_PLP_COMPACT_TILE - 1) / LFQ_PLP_COMPACT_TILE;
    const int64_t o_cov = 0, o_nb = o_cov + lfq_al(width * 4), o_cur = o_nb + lfq_al(width * 4), o_cidx = o_cur + lfq_al(width * 4),
                  o_tcol = o_cidx + lfq_al(width * 4), o_tobs = o_tcol + lfq_al(n_tiles * 8), o_tmax = o_tobs + lfq_al(n_tiles * 8),
                  o_tot = o_tmax + lfq_al(n_tiles * 4), o_cpos = o_tot + 256, total = o_cpos + lfq_al(width * 8);
    /* Everything goes to the main stream, behind the BAQ kernels if they are still running (the scatter pass reads their
     * lb bytes; pass 0 beside them was measured: 2 ms alone, 14 ms squeezed between wavefronts that hold 416 of a SIMD's
     * 512 registers, with the host waiting for its result).  Nothing waits for the scatter pass: the tracks are complete
     * in stream order (see the header) -- the host goes on with the indel tests while it runs. */
    hipStream_t ps = c->stream;
    LFQ_TRY(lfq_order_after_batch(c, c->stream));          /* the tracks of the previous call may still be a running batch's input */
    LFQ_TRY(grow(&c->d_plp_in, &c->plp_in_bytes, total));
    uint8_t *d = c->d_plp_in;
    LFQ_TRY_HIP(hipMemsetAsync(d + o_cov, 0, (size_t)(o_cidx - o_cov), ps));
    LfqPileupArgs A;
    memset(&A, 0, sizeof(A));
    /* position-sorted reads (the normal case): the column-major kernels; otherwise, if asked for, one thread per read + atomics
     * (as mpileup: bam_mplp_auto stops at a file that is not coordinate-sorted, plp.c:1406-1447) */
    LFQ_TRY(readset_pileup_view(c, rs, ps, true, &A));
    const bool sorted = A.pmax_end != nullptr;
    A.begin = region_begin;
    A.width = width;
    A.min_plp_bq = min_plp_bq;
    A.cov = (int32_t *)(d + o_cov);
    A.nb = (int32_t *)(d + o_nb);
    A.cursor = (int32_t *)(d + o_cur);
    LFQ_TRY(sorted ? lfq_launch_pileup_columns(A, 0, ps) : lfq_launch_pileup_count(A, ps));
    if (rs->bed) {
        /* plp.c:1412: a position outside every interval is no column, however many of the kept reads cover it */
        LFQ_TRY(lfq_launch_bed_mask_columns(rs->bed->tab, region_begin, width, A.cov, A.nb, ps));
    }
    /* columns from the counters on the device (lfq_launch_plp_compact_*): the host waits once, for three numbers */
    LfqPin<int64_t> tot(c, 4);
    LFQ_PIN_OK(tot);
    LFQ_TRY(lfq_launch_plp_compact_sums(A.cov, A.nb, width, (int64_t *)(d + o_tcol), (uint64_t *)(d + o_tobs),
                                        (int32_t *)(d + o_tmax), (int64_t *)(d + o_tot), ps));
    LFQ_TRY_HIP(hipMemcpyAsync(tot.data(), d + o_tot, 24, hipMemcpyDeviceToHost, ps));
    LFQ_TRY_HIP(hipStreamSynchronize(ps));
    const int64_t ncols = tot[0], n_obs = tot[1], max_obs = tot[2];
    const int64_t trk = lfq_al(n_obs + 32);
    const bool nt_packed = !c->plp_nt_bytes;
    const int64_t t_off = 0, t_ref = t_off + lfq_al((ncols + 1) * 8), t_cov = t_ref + lfq_al(ncols + 16), t_nb = t_cov + lfq_al(ncols * 4 + 16),
                  t_nt = t_nb + lfq_al(ncols * 4 + 16), t_bq = t_nt + trk, t_baq = t_bq + trk, t_mq = t_baq + trk,
                  t_sq = t_mq + trk, t_ntp = t_sq + (rs->has_sqb ? trk : 0), t_total = t_ntp + (nt_packed ? lfq_al(trk / 2 + 16) : 0);
    LFQ_TRY(grow(&c->d_plp_out, &c->plp_out_bytes, t_total));
    uint8_t *t = c->d_plp_out;
    LFQ_TRY_HIP(hipMemsetAsync(t + t_nt, 0, (size_t)(t_total - t_nt), ps));            /* the 16-byte tails are read */
    LFQ_TRY(lfq_launch_plp_compact_apply(A.cov, A.nb, width, region_begin, rs->d_ref, rs->ref_len, (const int64_t *)(d + o_tcol),
                                         (const uint64_t *)(d + o_tobs), (const int64_t *)(d + o_tot), (int32_t *)(d + o_cidx),
                                         (uint64_t *)(t + t_off), t + t_ref, (int32_t *)(t + t_cov), (int32_t *)(t + t_nb),
                                         (int64_t *)(d + o_cpos), ps));
    /* the columns' positions for the caller: copied on the context's own upload stream behind the apply kernel, so that the
     * wait for the copy below is not a wait for the scatter pass -- and not for another context's DP chain either (the DP
     * stream, which carried this copy before, is shared by the contexts of a device) */
    hipStream_t aux = ps;
    if (!lfq_knobs().single_stream) {
        if (!c->up_stream && hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking) != hipSuccess) {
            c->up_stream = nullptr;
            return LFQ_ERR_HIP;
        }
        aux = c->up_stream;
    }
    bool copy_pending = false;
    if (col_pos_out && ncols > 0) {
        if (!c->ev_apply) {
            LFQ_TRY_HIP(hipEventCreateWithFlags(&c->ev_apply, hipEventDisableTiming));     /* kept: destroyed with the context */
        }
        if (hipEventRecord(c->ev_apply, ps) != hipSuccess || (aux != ps && hipStreamWaitEvent(aux, c->ev_apply, 0) != hipSuccess)
            || hipMemcpyAsync(col_pos_out, d + o_cpos, (size_t)ncols * 8, hipMemcpyDeviceToHost, aux) != hipSuccess) {
            (void)hipStreamSynchronize(aux);
            return LFQ_ERR_HIP;
        }
        copy_pending = true;
    }
    A.col_index = (const int32_t *)(d + o_cidx);
    A.col_off = (const uint64_t *)(t + t_off);
    A.t_nt = t + t_nt;
    A.t_bq = t + t_bq;
    A.t_baq = t + t_baq;
    A.t_mq = t + t_mq;
    A.t_sq = rs->has_sqb ? t + t_sq : nullptr;
    int rc_sc = sorted ? lfq_launch_pileup_columns(A, 1, c->stream) : lfq_launch_pileup_scatter(A, c->stream);
    if (rc_sc == LFQ_OK && nt_packed) {
        /* the layout the count kernel reads 1.5 instead of 2 bytes per observation of (LFQ_TRACKS_NT_PACKED): the scatter
         * pass writes bytes (two lanes, often of two wavefronts, would share a byte), one streaming pass packs them */
        rc_sc = lfq_launch_pack_nt(t + t_nt, t + t_ntp, n_obs, c->stream);
    }
    if (copy_pending) {                             /* on every path: the copy into the caller's array is not left in flight */
        if (hipStreamSynchronize(aux) != hipSuccess && rc_sc == LFQ_OK) {
            rc_sc = LFQ_ERR_HIP;
        }
    }
    LFQ_TRY(rc_sc);
    /* (no wait for the tracks: what consumes them -- lfq_call_snvs_batch, lfq_pileup_skip_snv_columns, the uniq calls -- is
     * queued on the same stream; lfq_readset_destroy and lfq_synchronize wait for it) */
    out->nt = nt_packed ? t + t_ntp : t + t_nt;
    out->flags = nt_packed ? LFQ_TRACKS_NT_PACKED : 0;
    out->bq = t + t_bq;
    out->baq = t + t_baq;
    out->mq = t + t_mq;
    out->sq = rs->has_sqb ? t + t_sq : nullptr;
    out->col_off = (const uint64_t *)(t + t_off);
    out->ref_base = t + t_ref;
    out->coverage_plp = (const int32_t *)(t + t_cov);
    out->num_bases = (const int32_t *)(t + t_nb);
    c->d_plp_nb = (int32_t *)(t + t_nb);
    c->plp_ncols = ncols;
    out->ncols = ncols;
    out->max_col_obs = max_obs;
    return LFQ_OK;
}

/* ---- the pileup at a list of positions (`lofreq uniq` on a read set) ---------------------------------------------------
 * Count pass -> the per-site counts come back once (16 bytes a site; the binomial test needs them on the host anyway) ->
 * the column offsets, reference bases and the two count arrays of the tracks go down (21 bytes a site) -> scatter pass.  The
 * buffers are the context's own pair for this call family. */
int lfq_readset_sites_impl(lfq_ctx *c, lfq_readset *rs, const int64_t *site_pos, int64_t n_sites, int min_plp_bq,
                           const int64_t *key_off, const char *key_chars, const uint8_t *key_del, lfq_tracks *out,
                           int32_t *cov_out, int32_t *nb_out, int32_t *tails_out, int32_t *ev_out)
{
    if (!c || !rs || rs->c != c || !out || n_sites < 0 || (n_sites > 0 && !site_pos)
        || (rs->n > 0 && (!rs->seq || !rs->qual || !rs->mapq || !rs->reverse))) {
        return LFQ_ERR_INVALID;
    }
    memset(out, 0, sizeof(*out));
    memset(&c->sites_times, 0, sizeof(c->sites_times));
    if (n_sites == 0) {
        return LFQ_OK;
    }
    for (int64_t i = 0; i < n_sites; i++) {
        if (site_pos[i] < 0 || site_pos[i] >= rs->ref_len) {
            return LFQ_ERR_INVALID;
        }
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t ps = c->stream;
    LFQ_TRY(readset_upload_wait(rs, ps));
    /* the window search needs position-sorted reads, and the reference's -d acts on the reads of each 1-bp query: a cap
     * that drops a read of the region is not that rule */
    LFQ_TRY(readset_keep(c, rs));
    if (c->plp_max_depth != LFQ_NO_MAX_DEPTH && !rs->keep.empty() && rs->n_kept < (rs->bed ? rs->n_bed_kept : rs->n)) {
        return LFQ_ERR_INVALID;
    }
    LfqSitesArgs A;
    memset(&A, 0, sizeof(A));
    if (rs->bed) {
        /* `lofreq uniq` has no -l: every read, whatever the targets of the read set drop (the cap was decided on their survivors) */
        readset_view(rs, &A);
        LFQ_TRY(readset_pmax(c, rs, ps, false));
        A.pmax_end = rs->d_pmax;
    } else {
        LFQ_TRY(readset_pileup_view(c, rs, ps, false, &A));   /* (the cap decided above drops nothing: only the running maximum goes up) */
    }
    c->sites_times.n_sites = n_sites;
    const int64_t n = n_sites, n_key = key_off ? key_off[n] - key_off[0] : 0;
    /* what goes up in one copy: positions | key offsets | key sides | key letters; then the windows and the counts */
    const int64_t o_pos = 0, o_koff = o_pos + lfq_al(n * 8), o_kdel = o_koff + lfq_al((n + 1) * 8), o_kch = o_kdel + lfq_al(n),
                  o_win = o_kch + lfq_al(n_key + 1), o_cnt = o_win + lfq_al(n * 16), total = o_cnt + lfq_al(n * 16);
    LFQ_TRY(lfq_order_after_batch(c, ps));                 /* the tracks of the previous call may still be a running batch's input */
    LFQ_TRY(grow(&c->d_sites_in, &c->sites_in_bytes, total));
    uint8_t *d = c->d_sites_in;
    LfqPin<uint8_t> up(c, (size_t)o_win);
    LFQ_PIN_OK(up);
    memcpy(up.data() + o_pos, site_pos, (size_t)n * 8);
    if (key_off) {
        int64_t *ko = (int64_t *)(up.data() + o_koff);
        for (int64_t i = 0; i <= n; i++) {
            ko[i] = key_off[i] - key_off[0];
        }
        memcpy(up.data() + o_kdel, key_del, (size_t)n);
        if (n_key > 0) {
            memcpy(up.data() + o_kch, key_chars + key_off[0], (size_t)n_key);
        }
    }
    LFQ_TRY_HIP(hipMemcpyAsync(d, up.data(), (size_t)o_win, hipMemcpyHostToDevice, ps));
    A.n_sites = n;
    A.site_pos = (const int64_t *)(d + o_pos);
    A.min_plp_bq = min_plp_bq;
    if (key_off) {
        A.key_off = (const int64_t *)(d + o_koff);
        A.key_del = d + o_kdel;
        A.key_chars = d + o_kch;
    }
    A.counts = (int32_t *)(d + o_cnt);
    A.win = (int64_t *)(d + o_win);
    LfqPin<int32_t> h_cnt(c, (size_t)n * 4);
    LFQ_PIN_OK(h_cnt);
    LFQ_TRY(c->sites_t[0].begin(ps));
    LFQ_TRY(lfq_launch_pileup_sites(A, 0, ps));
    LFQ_TRY(c->sites_t[0].end(ps));
    c->sites_times.n_launches = 1;
    LFQ_TRY_HIP(hipMemcpyAsync(h_cnt.data(), A.counts, (size_t)n * 16, hipMemcpyDeviceToHost, ps));
    LFQ_TRY_HIP(hipStreamSynchronize(ps));
    const int32_t *h_cov = h_cnt.data(), *h_nb = h_cov + n, *h_tails = h_nb + n, *h_ev = h_tails + n;
    /* the header of the tracks, assembled here and sent down in one copy: offsets | reference bases | coverage_plp | num_bases */
    const int64_t t_off = 0, t_ref = t_off + lfq_al((n + 1) * 8), t_cov = t_ref + lfq_al(n + 16), t_nb = t_cov + lfq_al(n * 4 + 16),
                  t_nt = t_nb + lfq_al(n * 4 + 16);
    LfqPin<uint8_t> hdr(c, (size_t)t_nt);
    LFQ_PIN_OK(hdr);
    memset(hdr.data(), 0, (size_t)t_nt);
    uint64_t *h_off = (uint64_t *)(hdr.data() + t_off);
    int64_t n_obs = 0, max_obs = 0;
    for (int64_t i = 0; i < n; i++) {
        h_off[i] = (uint64_t)n_obs;
        n_obs += h_nb[i];
        max_obs = std::max<int64_t>(max_obs, h_nb[i]);
        hdr[(size_t)(t_ref + i)] = lfq_plp_ref_base(rs->ref, rs->ref_len, site_pos[i]);    /* as the region pileup */
    }
    h_off[n] = (uint64_t)n_obs;
    memcpy(hdr.data() + t_cov, h_cov, (size_t)n * 4);
    memcpy(hdr.data() + t_nb, h_nb, (size_t)n * 4);
    const int64_t trk = lfq_al(n_obs + 32);
    const int64_t t_bq = t_nt + trk, t_baq = t_bq + trk, t_mq = t_baq + trk, t_sq = t_mq + trk,
                  t_total = t_sq + (rs->has_sqb ? trk : 0);
    LFQ_TRY(grow(&c->d_sites_out, &c->sites_out_bytes, t_total));
    uint8_t *t = c->d_sites_out;
    LFQ_TRY_HIP(hipMemcpyAsync(t, hdr.data(), (size_t)t_nt, hipMemcpyHostToDevice, ps));
    for (int64_t o = t_nt; o < t_total; o += trk) {
        LFQ_TRY_HIP(hipMemsetAsync(t + o + n_obs, 0, (size_t)(trk - n_obs), ps));        /* the 16-byte tails are read */
    }
    if (n_obs > 0) {
        A.col_off = (const uint64_t *)(t + t_off);
        A.t_nt = t + t_nt;
        A.t_bq = t + t_bq;
        A.t_baq = t + t_baq;
        A.t_mq = t + t_mq;
        A.t_sq = rs->has_sqb ? t + t_sq : nullptr;
        LFQ_TRY(c->sites_t[1].begin(ps));
        LFQ_TRY(lfq_launch_pileup_sites(A, 1, ps));
        LFQ_TRY(c->sites_t[1].end(ps));
        c->sites_times.n_launches = 2;
    }
    c->sites_times.n_obs = n_obs;
    LFQ_TRY_HIP(hipStreamSynchronize(ps));                 /* (the header's staging block goes back to the pool on return) */
    for (int64_t i = 0; i < n; i++) {
        if (cov_out) cov_out[i] = h_cov[i];
        if (nb_out) nb_out[i] = h_nb[i];
        if (tails_out) tails_out[i] = h_tails[i];
        if (ev_out) ev_out[i] = h_ev[i];
    }
    out->nt = t + t_nt;
    out->bq = t + t_bq;
    out->baq = t + t_baq;
    out->mq = t + t_mq;
    out->sq = rs->has_sqb ? t + t_sq : nullptr;
    out->col_off = (const uint64_t *)(t + t_off);
    out->ref_base = t + t_ref;
    out->coverage_plp = (const int32_t *)(t + t_cov);
    out->num_bases = (const int32_t *)(t + t_nb);
    out->ncols = n;
    out->max_col_obs = max_obs;
    out->flags = 0;
    return LFQ_OK;
}

int lfq_readset_pileup_sites(lfq_ctx *c, lfq_readset *rs, const int64_t *site_pos, int64_t n_sites, int min_plp_bq,
                             lfq_tracks *out, int32_t *coverage_plp_out, int32_t *num_tails_out)
{
    return lfq_readset_sites_impl(c, rs, site_pos, n_sites, min_plp_bq, nullptr, nullptr, nullptr, out, coverage_plp_out,
                                  nullptr, num_tails_out, nullptr);
}

int lfq_last_sites_times(lfq_ctx *c, lfq_sites_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = c->sites_times;
    if (t->n_launches > 0) {
        LFQ_TRY_HIP(hipSetDevice(c->device));
        LFQ_TRY(c->sites_t[0].ms(&t->count_ms));
        if (t->n_launches > 1) {
            LFQ_TRY(c->sites_t[1].ms(&t->scatter_ms));
        }
    }
    return LFQ_OK;
}

/* compile_plp_col's indel fields for the reads of a region (plp.c:1019-1192): the sparse part (which read carries
 * which insertion / deletion where: straight from the CIGARs) is assembled here, the dense part (counts over all
 * pileup entries and the quality arrays of the reads WITHOUT an event at the event columns) by lfq_plp_indel_kernel */
int lfq_pileup_indel_columns(lfq_ctx *c, const lfq_pileup_reads *rd, const lfq_pileup_indel_tags *tg,
                             int64_t region_begin, int64_t region_end, int min_plp_idq,
                             const lfq_indel_columns **cols_out, int64_t *col_pos_out)
{
    if (!c || !rd || !cols_out || region_end < region_begin || rd->n_reads < 0
        || (rd->n_reads > 0 && (!rd->pos || !rd->cigar_off || !rd->cigar || !rd->seq_off || !rd->seq || !rd->mapq
                                || !rd->reverse || !rd->ref))) {
        return LFQ_ERR_INVALID;
    }
    lfq_readset *rs = nullptr;
    LFQ_TRY(lfq_readset_create(c, rd, tg, &rs));
    const int rc = lfq_readset_pileup_indels(c, rs, region_begin, region_end, min_plp_idq, cols_out, col_pos_out);
    lfq_readset_destroy(rs);            /* the columns live in the context */
    return rc;
}

/* the host arrays the indel pileup's host stages (lfq_plp_indel_host.h) read: tag bytes where the caller gave them (ai / ad
 * computed by lfq_readset_baq are fetched per event instead), the -d decision readset_pileup_view made */
static LfqPlpReads readset_plp_reads(const lfq_ctx *c, const lfq_readset *rs)
{
    LfqPlpReads R = {};
    R.pos = rs->pos; R.cigar_off = rs->cigar_off; R.seq_off = rs->seq_off; R.cigar = rs->cigar;
    R.seq = rs->seq; R.mapq = rs->mapq; R.reverse = rs->reverse; R.ref = rs->ref; R.ref_len = rs->ref_len;
    R.bi = rs->h_bi; R.bd = rs->h_bd; R.ai = rs->h_ai; R.ad = rs->h_ad; R.fl = rs->fl.data();
    R.sq = rs->h_sq ? rs->h_sq : (rs->sq32.empty() ? nullptr : rs->sq32.data());
    R.idq_mode = rs->idq_mode; R.idq_ins = rs->idq_ins; R.idq_del = rs->idq_del;
    R.keep = (readset_masked(c, rs) && rs->keep_valid && !rs->keep.empty()) ? rs->keep.data() : nullptr;
    return R;
}

int lfq_readset_pileup_indels(lfq_ctx *c, lfq_readset *rs, int64_t region_begin, int64_t region_end, int min_plp_idq,
                              const lfq_indel_columns **cols_out, int64_t *col_pos_out)
{
    if (!c || !rs || rs->c != c || !cols_out || region_end < region_begin || (rs->n > 0 && (!rs->mapq || !rs->reverse))) {
        return LFQ_ERR_INVALID;
    }
    if (c->plp_indel) {
        c->plp_indel->reset();              /* keeps the capacity: see LfqPin for what freeing a DMA target costs */
    } else {
        c->plp_indel = new LfqIndelColsOwned();
    }
    c->plp_ne_total[0] = c->plp_ne_total[1] = 0;
    LfqIndelColsOwned &O = *c->plp_indel;
    memset(&O.cols, 0, sizeof(O.cols));
    *cols_out = &O.cols;
    const int64_t n = rs->n, width = region_end - region_begin;
    if (n == 0 || width == 0) {
        for (LfqIndelColsOwned::Side &S : O.side) {
            for (auto *v : {&S.ne_off, &S.ev_off, &S.key_off, &S.rd_off}) {
                v->assign(1, 0);
            }
        }
        lfq_plp_publish(O);
        return LFQ_OK;
    }
    double tm[6] = {lfq_now_ms(), 0, 0, 0, 0, 0};
    /* 2. dense counters on the device */
    LFQ_TRY_HIP(hipSetDevice(c->device));
    /* Steps 2 and 3 read nothing lfq_readset_baq writes (of the flag bytes only the BI / BD bits, which its merge
     * kernel leaves as they are): while its kernels are still running they go to another stream and run beside them --
     * the BAQ kernels hold one wavefront per SIMD and 416 of its 512 registers, these kernels need 40. */
    hipStream_t ps = (rs->baq_pending && c->dps && !lfq_knobs().single_stream) ? c->dps : c->stream;
    (void)readset_pmax(c, rs, ps, true);    /* (its small upload is waited for on this stream: before the stream itself waits) */
    LFQ_TRY(readset_upload_wait(rs, ps));
    if (rs->ev_idq) {
        LFQ_TRY_HIP(hipStreamWaitEvent(ps, rs->ev_idq, 0));
    }
    const int64_t o_cnt = 0, o_cur = o_cnt + 9 * lfq_al(width * 4), o_off = o_cur + 2 * lfq_al(width * 4),
                  total = o_off + 2 * lfq_al(width * 8);
    LFQ_TRY(grow(&c->d_tmp[1], &c->tmp_bytes[1], total));
    uint8_t *d = c->d_tmp[1];
    /* an error from here on: the pinned blocks of this call may still be a copy's source or target */
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return rc;
    };
    if (hipMemsetAsync(d + o_cnt, 0, (size_t)(o_off - o_cnt), ps) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    LfqPlpIndelArgs A;
    memset(&A, 0, sizeof(A));
    A.begin = region_begin;
    A.width = width;
    A.min_plp_idq = min_plp_idq;
    int32_t **cnt[9] = {&A.cov, &A.tails, &A.non_indels, &A.n_ins, &A.n_dels, &A.non_ins_fw, &A.non_del_fw,
                        &A.ne_qsum[0], &A.ne_qsum[1]};
    /* the nine per-position counters come back into pinned memory (grow-only): DMA instead of a staged copy */
    int32_t *h[9] = {nullptr};
    LFQ_TRY(grow_pinned(&c->h_pin2, &c->pin2_bytes, 9 * lfq_al(width * 4)));
    for (int i = 0; i < 9; i++) {
        *cnt[i] = (int32_t *)(d + o_cnt + i * lfq_al(width * 4));
        h[i] = (int32_t *)(c->h_pin2 + i * lfq_al(width * 4));
    }
    /* not coordinate-sorted: refused like mpileup does (lfq_set_pileup_unsorted); -d cap: the kept reads only */
    int rc = readset_pileup_view(c, rs, ps, true, &A);
    if (rc == LFQ_OK) {
        rc = A.pmax_end ? lfq_launch_plp_indel_columns(A, 0, ps) : lfq_launch_plp_indel(A, 0, ps);
    }
    if (rc == LFQ_OK && rs->bed) {
        /* plp.c:1412, as in lfq_readset_pileup_snv: the coverage the host makes the columns from is 0 outside the targets */
        rc = lfq_launch_bed_mask_columns(rs->bed->tab, region_begin, width, A.cov, nullptr, ps);
    }
    const bool have_qsum = A.pmax_end != nullptr;       /* the column-major kernel sums the qualities itself */
    for (int i = 0; i < (have_qsum ? 9 : 7) && rc == LFQ_OK; i++) {
        if (hipMemcpyAsync(h[i], *cnt[i], (size_t)width * 4, hipMemcpyDeviceToHost, ps) != hipSuccess) {
            rc = LFQ_ERR_HIP;
        }
    }
    if (rc != LFQ_OK) {
        return fail(rc);
    }
    /* 1. events from the CIGARs, every thread those of its reads, then merged (host arrays only: runs while the counter
     * kernel of step 2 does) */
    const LfqPlpReads R = readset_plp_reads(c, rs);
    std::vector<LfqPlpEv> evs, evs_part[LFQ_HOST_PARTS];
    lfq_for_reads(n, [&](int64_t r_begin, int64_t r_end, int part) {
        lfq_plp_scan_events(R, r_begin, r_end, region_begin, region_end, min_plp_idq, evs_part[part]);
    });
    lfq_plp_merge_events(evs_part, LFQ_HOST_PARTS, evs);
    if (rs->bed) {
        /* an event belongs to the column of its position: outside the targets there is none (the host copy of the same table) */
        const LfqBedTab tab = rs->bed->host.tab();
        evs.erase(std::remove_if(evs.begin(), evs.end(), [&](const LfqPlpEv &e) { return !lfq_bed_tab_overlap(tab, e.pos, e.pos + 1); }),
                  evs.end());
    }
    /* 4a. the event tables, part by part, while the counter kernel is still on its way (it waits for BI / BD, the end of
     * the upload): they need the events and the caller's arrays, nothing from the device */
    const int n_parts = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min<long>(std::max<long>(lfq_knobs().host_loop_threads, 1), LFQ_HOST_PARTS), evs.size() / (size_t)std::max<int64_t>(lfq_knobs().host_par_min / 48, 1)));
    const std::vector<size_t> cut = lfq_plp_table_cuts(evs, n_parts);
    std::vector<LfqPlpPartTables> pt((size_t)n_parts);
    lfq_run_parts(n_parts, [&](int t) { lfq_plp_build_tables(R, evs, cut[(size_t)t], cut[(size_t)t + 1], region_begin, pt[(size_t)t]); });
    LfqPlpTables T;
    lfq_plp_append_tables(pt, O, T);
    tm[1] = lfq_now_ms();
    if (hipStreamSynchronize(ps) != hipSuccess) {
        return fail(LFQ_ERR_HIP);
    }
    tm[2] = lfq_now_ms();
    /* 3. columns = covered positions; quality arrays of the reads without an event at the event positions */
    LfqPin<int64_t> pos_off_ins(c, (size_t)width), pos_off_del(c, (size_t)width);      /* DMA sources: pinned */
    if (!pos_off_ins.ok() || !pos_off_del.ok()) {
        return fail(LFQ_ERR_NOMEM);
    }
    int64_t *const pos_off[2] = {pos_off_ins.data(), pos_off_del.data()};
    LfqVec<int32_t> col_of((size_t)width);      /* (col_of and pos_off: every position is written by the second pass) */
    const bool host_arrays = c->indel_host_arrays || !have_qsum;   /* device-only needs the sums from the kernel */
    std::vector<uint8_t> has_ev;
    lfq_plp_mark_events(evs, region_begin, width, c->indel_all_columns != 0, has_ev);   /* lfq_set_indel_arrays_all_columns */
    LfqPlpPartCount pc[LFQ_HOST_PARTS + 1] = {};
    int parts = 1;
    lfq_for_reads(width, [&](int64_t p0, int64_t p1, int part) { pc[part + 1] = lfq_plp_cols_count(h, has_ev, p0, p1); }, &parts);
    lfq_plp_cols_alloc(O, pc, parts, have_qsum);
    lfq_for_reads(width, [&](int64_t p0, int64_t p1, int part) {
        lfq_plp_cols_fill(R, h, has_ev, region_begin, p0, p1, pc[part], have_qsum, O, col_of.data(), pos_off, col_pos_out);
    });
    const int64_t ne_total[2] = {pc[parts].ne[0], pc[parts].ne[1]}, ne_all = ne_total[0] + ne_total[1];
    if (ne_all > 0 && grow(&c->d_plp_ne, &c->plp_ne_cap, ne_all * 2) != LFQ_OK) {
        return fail(LFQ_ERR_NOMEM);
    }
    if (ne_all > 0) {
        int16_t *d_ne = c->d_plp_ne;
        for (int sd = 0; sd < 2 && rc == LFQ_OK; sd++) {
            uint8_t *d_off = d + o_off + sd * lfq_al(width * 8);
            A.ne_off[sd] = (const int64_t *)d_off;
            A.cursor[sd] = (int32_t *)(d + o_cur + sd * lfq_al(width * 4));
            if (hipMemcpyAsync(d_off, pos_off[sd], (size_t)width * 8, hipMemcpyHostToDevice, ps) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
        }
        A.ne_q[0] = d_ne;
        A.ne_mq[0] = d_ne + ne_total[0];
        A.ne_q[1] = d_ne + 2 * ne_total[0];
        A.ne_mq[1] = d_ne + 2 * ne_total[0] + ne_total[1];
        if (rc == LFQ_OK) {
            rc = A.pmax_end ? lfq_launch_plp_indel_columns(A, 1, ps) : lfq_launch_plp_indel(A, 1, ps);
        }
        for (int sd = 0; sd < 2 && rc == LFQ_OK && host_arrays; sd++) {
            O.side[sd].ne_q.resize((size_t)ne_total[sd]);
            O.side[sd].ne_mq.resize((size_t)ne_total[sd]);
            if (ne_total[sd] > 0
                && (hipMemcpyAsync(O.side[sd].ne_q.data(), A.ne_q[sd], (size_t)ne_total[sd] * 2, hipMemcpyDeviceToHost, ps) != hipSuccess
                    || hipMemcpyAsync(O.side[sd].ne_mq.data(), A.ne_mq[sd], (size_t)ne_total[sd] * 2, hipMemcpyDeviceToHost, ps) != hipSuccess)) {
                rc = LFQ_ERR_HIP;
            }
        }
        if (rc != LFQ_OK) {
            return fail(rc);
        }
        /* (waited for behind the event tables below) */
    }
    tm[3] = lfq_now_ms();
    /* ai / ad of the event reads when lfq_readset_baq left them on the device: the gather is queued behind the BAQ
     * kernels on their stream and lands in pinned memory; nothing waits for it until the ev_off entries and the consensus
     * flags -- which need neither ai / ad nor the tag bits of the reads -- are there (that host work used to start
     * when the last BAQ kernel had ended: 7 ms of an idle GPU per region). */
    LfqPin<int64_t> idx(c, evs.size());
    LfqPin<uint8_t> g_pin(c, 2 * evs.size());
    const bool gather_aq = rs->has_idaq && !evs.empty();
    if (gather_aq) {
        const int64_t ne = (int64_t)evs.size();
        if (!idx.ok() || !g_pin.ok() || grow(&c->d_tmp[2], &c->tmp_bytes[2], ne * 10) != LFQ_OK) {
            return fail(LFQ_ERR_NOMEM);
        }
        lfq_plp_gather_index(R, evs, idx.data());
        uint8_t *dg = c->d_tmp[2];
        if (hipMemcpyAsync(dg, idx.data(), (size_t)ne * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess
            || lfq_launch_gather2(rs->d_ai, rs->d_ad, (const int64_t *)dg, ne, dg + ne * 8, dg + ne * 9, c->stream) != LFQ_OK
            || hipMemcpyAsync(g_pin.data(), dg + ne * 8, (size_t)ne * 2, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
            return fail(LFQ_ERR_HIP);
        }
    }
    /* the quality arrays stay resident (c->d_plp_ne): lfq_call_indels_batch builds its pseudo-columns from them on the device */
    c->plp_ne_total[0] = ne_total[0];
    c->plp_ne_total[1] = ne_total[1];
    tm[4] = lfq_now_ms();
    /* 4. the running event counts per column, and the consensus flags where the counter kernel summed the non-event
     * qualities: while the scatter pass, the BAQ kernels and the gather run */
    if (!lfq_plp_fill_ev_off(T, col_of.data(), O)) {
        return fail(LFQ_ERR_INVALID);
    }
    if (have_qsum) {
        lfq_plp_cons_flags(T, col_of.data(), true, O);
    }
    /* 4b. the scatter pass, the BAQ kernels and the gather behind them: the alignment qualities of the event reads; from here
     * on the ai / ad bits of rs->fl (R.fl) are valid */
    if (hipStreamSynchronize(ps) != hipSuccess || (gather_aq && hipStreamSynchronize(c->stream) != hipSuccess)
        || readset_baq_wait(rs) != LFQ_OK) {
        return LFQ_ERR_HIP;
    }
    lfq_plp_fill_rd_aq(R, evs, T, gather_aq ? g_pin.data() : nullptr, gather_aq ? g_pin.data() + evs.size() : nullptr, O);
    if (!have_qsum) {
        lfq_plp_cons_flags(T, col_of.data(), false, O);     /* ... else over the quality arrays the scatter pass brought back */
    }
    tm[5] = lfq_now_ms();
    if (lfq_timing_on) {
        fprintf(stderr, "[lfq timing] indel pileup: counters queued + events %.1f  wait %.1f  columns + scatter queued %.1f  gather queued %.1f  tables + consensus + wait + ai / ad %.1f ms\n",
                tm[1] - tm[0], tm[2] - tm[1], tm[3] - tm[2], tm[4] - tm[3], tm[5] - tm[4]);
    }
    lfq_plp_publish(O);         /* 6. (O.ne_qsum stays for lfq_readset_plp_summary: the key of a consensus indel) */
    return LFQ_OK;
}

/* ---- plp_summary's header line (lofreq_call.c:445-459) for the columns of a region -------------------------------------------
 * The indel side (coverage_plp, num_tails, num_ins, num_dels, hrun, the event tables and the non-event quality sums) is the
 * indel pileup's of the same read set and region, run here; lfq_plp_summary_kernel adds the strand-resolved base counts,
 * num_heads and the consensus base on the columns it found; the key of a consensus indel is picked from the event tables here
 * (plp.c:1231-1268: the first event of a side whose quality sum is strictly greatest, against the side's non-event sum; an
 * insertion before a deletion). */
static const double *summary_incr_table()
{
    static double tab[94];
    static const bool done = [] {
        for (int q = 0; q < 94; q++) {
            double v = 1.0 - pow(10.0, -1.0 * q / 10.0);       /* 1.0 - PHREDQUAL_TO_PROB(bq), plp.c:999 */
            if (v == 0.0) {
                v = DBL_MIN;                                    /* plp.c:1003-1005 */
            }
            tab[q] = v;
        }
        return true;
    }();
    (void)done;
    return tab;
}

int lfq_readset_plp_summary(lfq_ctx *c, lfq_readset *rs, int64_t region_begin, int64_t region_end, int min_plp_bq,
                            int min_plp_idq, const lfq_plp_summary **out)
{
    if (!c || !rs || rs->c != c || !out || region_end < region_begin || region_begin < 0 || region_end > rs->ref_len
        || min_plp_bq < 0 || (rs->n > 0 && (!rs->seq || !rs->qual || !rs->mapq || !rs->reverse))) {
        return LFQ_ERR_INVALID;
    }
    if (!c->plp_sum) {
        c->plp_sum = new LfqSummaryOwned();
    }
    LfqSummaryOwned &S = *c->plp_sum;
    memset(&S.sum, 0, sizeof(S.sum));
    memset(&c->sum_times, 0, sizeof(c->sum_times));
    S.col_pos.clear();
    S.key_chars.clear();
    S.key_off.assign(1, 0);
    S.ref_base.clear();
    S.cons_kind.clear();
    for (auto *v : {&S.n_ins, &S.n_dels, &S.hrun, &S.cov}) {
        v->clear();
    }
    auto publish = [&S, out]() {
        lfq_plp_summary &P = S.sum;
        P.ncols = (int64_t)S.col_pos.size();
        P.col_pos = S.col_pos.data();
        P.ref_base = S.ref_base.data();
        P.fw = P.rv = P.num_heads = P.num_tails = nullptr;      /* (ncols > 0: set to the pinned block by the caller) */
        P.num_ins = S.n_ins.data();
        P.num_dels = S.n_dels.data();
        P.hrun = S.hrun.data();
        P.coverage_plp = S.cov.data();
        P.cons_kind = S.cons_kind.data();
        P.cons_nt = nullptr;
        P.cons_key_off = S.key_off.data();
        S.key_chars.push_back('\0');
        P.cons_key_chars = S.key_chars.data();
        *out = &P;
        return LFQ_OK;
    };
    const int64_t width = region_end - region_begin;
    if (rs->n == 0 || width == 0) {
        return publish();
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t ps = c->stream;
    LFQ_TRY(readset_upload_wait(rs, ps));
    LFQ_TRY(readset_pmax(c, rs, ps, false));    /* the window search needs position-sorted reads (lfq_set_pileup_unsorted does not apply) */
    /* the indel side: the context's current lfq_indel_columns are this region's from here on */
    const lfq_indel_columns *ic = nullptr;
    S.col_pos.resize((size_t)width);
    const int rc_ind = lfq_readset_pileup_indels(c, rs, region_begin, region_end, min_plp_idq, &ic, S.col_pos.data());
    if (rc_ind != LFQ_OK) {
        S.col_pos.clear();
        return rc_ind;
    }
    const int64_t ncols = ic->ncols;
    S.col_pos.resize((size_t)ncols);
    if (ncols == 0) {
        return publish();
    }
    const LfqIndelColsOwned &O = *c->plp_indel;
    if (O.ne_qsum[0].size() != (size_t)ncols || O.ne_qsum[1].size() != (size_t)ncols) {
        return LFQ_ERR_INVALID;             /* (cannot happen: sorted reads go to the kernel that sums the qualities) */
    }
    /* what goes up in one copy: column positions | increment table; what the kernel writes and one copy brings back into pinned
     * memory, where the struct points at it: fw | rv | heads | tails | consensus letter | path */
    const int64_t o_pos = 0, o_incr = o_pos + lfq_al(ncols * 8), o_cnt = o_incr + lfq_al(94 * 8), o_rv = o_cnt + lfq_al(ncols * 20),
                  o_heads = o_rv + lfq_al(ncols * 20), o_tails = o_heads + lfq_al(ncols * 4), o_cons = o_tails + lfq_al(ncols * 4),
                  o_ord = o_cons + lfq_al(ncols), total = o_ord + lfq_al(ncols);
    LFQ_TRY(grow(&c->d_sum, &c->sum_bytes, total));
    uint8_t *d = c->d_sum;
    LFQ_TRY(grow_pinned(&c->h_sum, &c->h_sum_bytes, total - o_cnt));
    const uint8_t *h = c->h_sum - o_cnt;                    /* h + o_x: where the device's d + o_x lands */
    /* the reads, with the -d decision both pileups share (the sorted-or-refused answer was needed before the indel side ran, so
     * readset_pmax is called there; here, before the first copy is queued: nothing below returns with one in flight) */
    LfqSummaryArgs A;
    memset(&A, 0, sizeof(A));
    LFQ_TRY(readset_pileup_view(c, rs, ps, false, &A));
    LfqPin<uint8_t> up(c, (size_t)o_cnt);
    LFQ_PIN_OK(up);
    memcpy(up.data() + o_pos, S.col_pos.data(), (size_t)ncols * 8);
    memcpy(up.data() + o_incr, summary_incr_table(), 94 * 8);
    int rc = hipMemcpyAsync(d, up.data(), (size_t)o_cnt, hipMemcpyHostToDevice, ps) == hipSuccess ? LFQ_OK : LFQ_ERR_HIP;
    A.n_cols = ncols;
    A.col_pos = (const int64_t *)(d + o_pos);
    A.min_plp_bq = min_plp_bq;
    A.incr = (const double *)(d + o_incr);
    A.fw = (int32_t *)(d + o_cnt);
    A.rv = (int32_t *)(d + o_rv);
    A.heads = (int32_t *)(d + o_heads);
    A.tails = (int32_t *)(d + o_tails);
    A.cons_nt = d + o_cons;
    A.ordered = d + o_ord;
    if (rc == LFQ_OK) {
        rc = c->sum_t.begin(ps);
    }
    if (rc == LFQ_OK) {
        rc = lfq_launch_plp_summary(A, ps);
    }
    if (rc == LFQ_OK && (c->sum_t.end(ps) != LFQ_OK
                         || hipMemcpyAsync(c->h_sum, d + o_cnt, (size_t)(total - o_cnt), hipMemcpyDeviceToHost, ps) != hipSuccess)) {
        rc = LFQ_ERR_HIP;
    }
    if (rc == LFQ_OK) {
        c->sum_times.n_launches = 1;
        c->sum_times.n_cols = ncols;
    }
    /* the indel side's share of the struct and the consensus indels, while the kernel runs */
    S.cons_kind.assign((size_t)ncols, 0);
    S.key_off.resize((size_t)ncols + 1);
    S.ref_base.assign(ic->ref_base, ic->ref_base + ncols);
    S.n_ins.assign(ic->num_ins, ic->num_ins + ncols);
    S.n_dels.assign(ic->num_dels, ic->num_dels + ncols);
    S.hrun.assign(ic->hrun, ic->hrun + ncols);
    S.cov.assign(ic->coverage_plp, ic->coverage_plp + ncols);
    for (int64_t col = 0; col < ncols; col++) {
        int64_t best_ev[2];                                         /* consensus indel, plp.c:1231-1268 */
        for (int sd = 0; sd < 2; sd++) {
            const lfq_indel_side &T = ic->side[sd];
            best_ev[sd] = lfq_plp_cons_event(T.ev_off, T.rd_off, T.rd_q, col, O.ne_qsum[sd][(size_t)col]);
        }
        const int sd = best_ev[0] >= 0 ? 0 : (best_ev[1] >= 0 ? 1 : -1);
        if (sd >= 0) {
            const lfq_indel_side &T = ic->side[sd];
            S.cons_kind[(size_t)col] = (uint8_t)(sd + 1);
            S.key_chars.insert(S.key_chars.end(), T.key_chars + T.key_off[best_ev[sd]], T.key_chars + T.key_off[best_ev[sd] + 1]);
        }
        S.key_off[(size_t)col + 1] = (int64_t)S.key_chars.size();
    }
    if (hipStreamSynchronize(ps) != hipSuccess) {       /* on every path: `up` goes back to the pool on return */
        rc = LFQ_ERR_HIP;
    }
    LFQ_TRY(rc);
    int64_t n_ordered = 0;
    for (int64_t col = 0; col < ncols; col++) {
        n_ordered += (h + o_ord)[col];
    }
    c->sum_times.n_ordered = n_ordered;
    publish();
    S.sum.fw = (const int32_t *)(h + o_cnt);
    S.sum.rv = (const int32_t *)(h + o_rv);
    S.sum.num_heads = (const int32_t *)(h + o_heads);
    S.sum.num_tails = (const int32_t *)(h + o_tails);
    S.sum.cons_nt = h + o_cons;
    return LFQ_OK;
}

int lfq_last_summary_times(lfq_ctx *c, lfq_summary_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = c->sum_times;
    if (t->n_launches > 0) {
        LFQ_TRY_HIP(hipSetDevice(c->device));
        LFQ_TRY(c->sum_t.ms(&t->kernel_ms));
    }
    return LFQ_OK;
}

/* ---- the nucleotide lines of plp_summary (lofreq_call.c:460-489): the tracks' bytes grouped per column --------------------------
 * One buffer on the device, [uploaded slice of host tracks |] nt_off | bq | baq | mq | sq, whose output part one copy brings into
 * pinned memory, where the struct points at it. */
int lfq_plp_quals_from_tracks(lfq_ctx *c, const lfq_tracks *tr, int tracks_on_device, int64_t col_begin, int64_t col_end,
                              const lfq_plp_quals **out)
{
    if (!c || !tr || !out) {
        return LFQ_ERR_INVALID;
    }
    if (col_begin < 0 || col_end < col_begin || col_end > tr->ncols || (tr->flags & LFQ_TRACKS_NT_PACKED)) {
        return LFQ_ERR_INVALID;
    }
    const int64_t ncols = col_end - col_begin;
    if (ncols > 0 && (!tr->col_off || !tr->nt || !tr->bq || !tr->mq)) {
        return LFQ_ERR_INVALID;
    }
    lfq_plp_quals &Q = c->plp_quals;
    memset(&Q, 0, sizeof(Q));
    memset(&c->pq_times, 0, sizeof(c->pq_times));
    Q.ncols = ncols;
    Q.col_begin = col_begin;
    c->pq_times.n_cols = ncols;
    *out = &Q;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    hipStream_t ps = c->stream;
    /* the range's first and last offset: how large the output is */
    uint64_t ends[2] = {0, 0};
    if (ncols > 0 && tracks_on_device) {
        LfqPin<uint64_t> e2(c, 2);
        LFQ_PIN_OK(e2);
        int rc = LFQ_OK;
        if (hipMemcpyAsync(e2.data(), tr->col_off + col_begin, 8, hipMemcpyDeviceToHost, ps) != hipSuccess
            || hipMemcpyAsync(e2.data() + 1, tr->col_off + col_end, 8, hipMemcpyDeviceToHost, ps) != hipSuccess) {
            rc = LFQ_ERR_HIP;
        }
        if (hipStreamSynchronize(ps) != hipSuccess) {
            rc = LFQ_ERR_HIP;
        }
        LFQ_TRY(rc);
        ends[0] = e2[0];
        ends[1] = e2[1];
    } else if (ncols > 0) {
        ends[0] = tr->col_off[col_begin];
        ends[1] = tr->col_off[col_end];
    }
    if (ends[1] < ends[0]) {
        return LFQ_ERR_INVALID;
    }
    const int64_t n_obs = (int64_t)(ends[1] - ends[0]);
    c->pq_times.n_obs = n_obs;
    const int64_t n_off = 5 * ncols + 1;
    const bool has_baq = tr->baq != nullptr, has_sq = tr->sq != nullptr;
    /* output: nt_off | bq | baq | mq | sq */
    const int64_t r_off = 0, r_bq = r_off + lfq_al(n_off * 8), r_baq = r_bq + lfq_al(n_obs), r_mq = r_baq + (has_baq ? lfq_al(n_obs) : 0),
                  r_sq = r_mq + lfq_al(n_obs), r_total = r_sq + (has_sq ? lfq_al(n_obs) : 0);
    LFQ_TRY(grow_pinned(&c->h_pq, &c->h_pq_bytes, r_total));
    uint8_t *h = c->h_pq;
    int64_t *h_off = (int64_t *)(h + r_off);
    Q.nt_off = h_off;
    Q.bq = h + r_bq;
    Q.baq = has_baq ? h + r_baq : nullptr;
    Q.mq = h + r_mq;
    Q.sq = has_sq ? h + r_sq : nullptr;
    if (n_obs == 0) {                       /* an empty range, or one without observations: nothing to launch */
        for (int64_t i = 0; i < n_off; i++) {
            h_off[i] = 0;
        }
        return LFQ_OK;
    }
    /* host tracks: col_off | nt | bq | baq | mq | sq of the range go up in front of the output */
    const int64_t u_off = 0, u_nt = u_off + lfq_al((ncols + 1) * 8), u_bq = u_nt + lfq_al(n_obs), u_baq = u_bq + lfq_al(n_obs),
                  u_mq = u_baq + (has_baq ? lfq_al(n_obs) : 0), u_sq = u_mq + lfq_al(n_obs), u_total = u_sq + (has_sq ? lfq_al(n_obs) : 0);
    const int64_t o_out = tracks_on_device ? 0 : u_total;
    LFQ_TRY(grow(&c->d_pq, &c->pq_bytes, o_out + r_total));
    uint8_t *d = c->d_pq;
    LfqPlpGroupArgs A;
    memset(&A, 0, sizeof(A));
    A.n_cols = ncols;
    int rc = LFQ_OK;
    if (tracks_on_device) {
        A.nt = tr->nt;
        A.bq = tr->bq;
        A.baq = tr->baq;
        A.mq = tr->mq;
        A.sq = tr->sq;
        A.col_off = tr->col_off + col_begin;
        A.in_shift = 0;
    } else {
        auto up = [&](int64_t off, const void *src, int64_t bytes) {
            if (rc == LFQ_OK && src && bytes > 0
                && hipMemcpyAsync(d + off, src, (size_t)bytes, hipMemcpyHostToDevice, ps) != hipSuccess) {
                rc = LFQ_ERR_HIP;
            }
        };
        up(u_off, tr->col_off + col_begin, (ncols + 1) * 8);
        up(u_nt, tr->nt + ends[0], n_obs);
        up(u_bq, tr->bq + ends[0], n_obs);
        up(u_baq, has_baq ? tr->baq + ends[0] : nullptr, n_obs);
        up(u_mq, tr->mq + ends[0], n_obs);
        up(u_sq, has_sq ? tr->sq + ends[0] : nullptr, n_obs);
        A.nt = d + u_nt;
        A.bq = d + u_bq;
        A.baq = has_baq ? d + u_baq : nullptr;
        A.mq = d + u_mq;
        A.sq = has_sq ? d + u_sq : nullptr;
        A.col_off = (const uint64_t *)(d + u_off);
        A.in_shift = ends[0];
    }
    A.nt_off = (int64_t *)(d + o_out + r_off);
    A.o_bq = d + o_out + r_bq;
    A.o_baq = has_baq ? d + o_out + r_baq : nullptr;
    A.o_mq = d + o_out + r_mq;
    A.o_sq = has_sq ? d + o_out + r_sq : nullptr;
    if (rc == LFQ_OK) {
        rc = c->pq_t.begin(ps);
    }
    if (rc == LFQ_OK) {
        rc = lfq_launch_plp_group(A, ps);
    }
    if (rc == LFQ_OK && (c->pq_t.end(ps) != LFQ_OK
                         || hipMemcpyAsync(h, d + o_out, (size_t)r_total, hipMemcpyDeviceToHost, ps) != hipSuccess)) {
        rc = LFQ_ERR_HIP;
    }
    if (rc == LFQ_OK) {
        c->pq_times.n_launches = 1;
    }
    if (hipStreamSynchronize(ps) != hipSuccess) {       /* on every path: the caller's host tracks may still be a copy's source */
        rc = LFQ_ERR_HIP;
    }
    return rc;
}

int lfq_last_plp_quals_times(lfq_ctx *c, lfq_plp_quals_times *t)
{
    if (!c || !t) {
        return LFQ_ERR_INVALID;
    }
    *t = c->pq_times;
    if (t->n_launches > 0) {
        LFQ_TRY_HIP(hipSetDevice(c->device));
        LFQ_TRY(c->pq_t.ms(&t->kernel_ms));
    }
    return LFQ_OK;
}

int lfq_source_qual_batch(lfq_ctx *c, const lfq_baq_reads *rd, int def_nm_q, int min_bq, const uint8_t *ign,
                          int32_t *sq_out, uint8_t *sq_byte)
{
    if (!c || !rd || !sq_out || rd->n_reads < 0 || def_nm_q > 255
        || (rd->n_reads > 0 && (!rd->pos || !rd->cigar_off || !rd->cigar || !rd->seq_off || !rd->seq || !rd->qual
                                || !rd->ref))) {
        return LFQ_ERR_INVALID;
    }
    if (rd->n_reads == 0) {
        return LFQ_OK;
    }
    lfq_readset *rs = nullptr;
    LFQ_TRY(readset_from_baq_reads(c, rd, &rs));
    const int rc = lfq_readset_source_qual(c, rs, def_nm_q, min_bq, ign, sq_out);
    if (rc == LFQ_OK && sq_byte) {
        for (int64_t r = 0; r < rd->n_reads; r++) {
            const int q = sq_out[r];
            sq_byte[r] = (uint8_t)(q < 0 ? 0 : (q > 254 ? 254 : q));
        }
    }
    lfq_readset_destroy(rs);
    return rc;
}

int lfq_readset_source_qual(lfq_ctx *c, lfq_readset *rs, int def_nm_q, int min_bq, const uint8_t *ign, int32_t *sq_out)
{
    if (!c || !rs || rs->c != c || def_nm_q > 255 || (rs->n > 0 && !rs->qual)) {
        return LFQ_ERR_INVALID;
    }
    const lfq_readset *rd = rs;
    const int64_t n = rs->n;
    if (n == 0) {
        return LFQ_OK;
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(readset_upload_wait(rs));
    int64_t max_ops = 0;                                /* bound of K: one operation per base or CIGAR element */
    for (int64_t r = 0; r < n; r++) {
        max_ops = std::max<int64_t>(max_ops, (rd->seq_off[r + 1] - rd->seq_off[r]) + (rd->cigar_off[r + 1] - rd->cigar_off[r]));
    }
    const int n_blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, (int64_t)c->n_cu * 2));
    const int64_t scratch_cells = max_ops + 1 > LFQ_SRCQ_LDS_CELLS ? max_ops + 1 : 0;
    const int64_t o_ign = 0, o_prob = o_ign + (ign ? lfq_al(rd->ref_len) : 0), o_st = o_prob + lfq_al(n * 8), o_scr = o_st + lfq_al(n),
                  total = o_scr + (int64_t)n_blocks * 4 * 2 * scratch_cells * 8;
    uint8_t *d = nullptr;
    if (hipMalloc((void **)&d, (size_t)total) != hipSuccess) {
        return LFQ_ERR_NOMEM;
    }
    int rc = LFQ_OK;
    LfqPin<double> prob(c, (size_t)n);
    LfqPin<uint8_t> st(c, (size_t)n);
    if (!prob.ok() || !st.ok()) {
        rc = LFQ_ERR_NOMEM;
    }
    if (ign && hipMemcpyAsync(d + o_ign, ign, (size_t)rd->ref_len, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        rc = LFQ_ERR_HIP;
    }
    if (rc == LFQ_OK) {
        LfqSrcqArgs A;
        memset(&A, 0, sizeof(A));
        readset_view(rs, &A);
        A.ign = ign ? d + o_ign : nullptr;
        A.nonmatch_qual = def_nm_q;
        A.min_bq = min_bq;
        A.scratch = scratch_cells ? (double *)(d + o_scr) : nullptr;
        A.scratch_cells = scratch_cells;
        A.prob = (double *)(d + o_prob);
        A.status = d + o_st;
        rc = lfq_launch_srcq(A, c->d_luts, n_blocks, c->stream);
    }
    if (rc == LFQ_OK
        && (hipMemcpyAsync(prob.data(), d + o_prob, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess
            || hipMemcpyAsync(st.data(), d + o_st, (size_t)n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)) {
        rc = LFQ_ERR_HIP;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == LFQ_OK) {
        rc = LFQ_ERR_HIP;
    }
    (void)hipFree(d);
    if (rc != LFQ_OK) {
        return rc;
    }
    const int perfect = (int)(-10.0L * log10l(LDBL_MIN));       /* PROB_TO_PHREDQUAL(LDBL_MIN) = 49314, plp.c:521 */
    rs->sq32.resize((size_t)n);
    LfqPin<uint8_t> sqb(c, (size_t)n);
    LFQ_PIN_OK(sqb);
    for (int64_t r = 0; r < n; r++) {
        int q;
        if (st[(size_t)r] == LFQ_SRCQ_NA) {
            q = -1;
        } else if (st[(size_t)r] == LFQ_SRCQ_PERFECT) {
            q = perfect;
        } else {
            const double x = 1.0 - prob[(size_t)r];             /* PROB_TO_PHREDQUAL(1.0 - src_prob), plp.c:567 */
            /* log10l(0) = -inf and a negative argument gives NaN: the x86-64 long double -> int conversion
             * of either is INT_MIN ("integer indefinite"); mplp_func then stores 0 */
            q = (x > 0.0) ? (int)(-10.0L * log10l((long double)x)) : INT32_MIN;
        }
        if (sq_out) {
            sq_out[r] = q;
        }
        rs->sq32[(size_t)r] = q < 0 ? 0 : q;                    /* what the sq tag holds (plp.c:731-734) */
        sqb[(size_t)r] = (uint8_t)(q < 0 ? 0 : (q > 254 ? 254 : q));
    }
    /* the byte of the packed sq track, resident for lfq_readset_pileup_snv */
    LFQ_TRY_HIP(hipMemcpy(rs->d_sqb, sqb.data(), (size_t)n, hipMemcpyHostToDevice));
    rs->has_sqb = true;
    return LFQ_OK;
}

/* `lofreq viterbi` on the resident reads: a NEW read set of the same reads with the realigned positions and CIGARs, stably
 * sorted by new position; `rs` itself is only read.  The realignment is lfq_viterbi_batch's (lfq_viterbi.hip) with query, q2def
 * and windows gathered from the device copy; the per-base arrays of the new set are written on the device from those of `rs`,
 * its host views are copies it owns (LfqReadsetOwned), so that it needs neither `rs` nor the caller's arrays afterwards. */
int lfq_readset_viterbi(lfq_ctx *c, lfq_readset *rs, int def_qual, lfq_readset **out, const lfq_viterbi_result **result_out,
                        const int64_t **order_out)
{
    if (result_out) *result_out = nullptr;
    if (order_out) *order_out = nullptr;
    if (out) *out = nullptr;
    if (!c || !rs || rs->c != c || !out || def_qual > 93 || (rs->n > 0 && (!rs->seq || !rs->qual))) {
        return LFQ_ERR_INVALID;
    }
    /* what depends on the alignment cannot be carried over: lb, ai / ad, source quality, BI / BD computed from the CIGARs */
    if (rs->has_lb || rs->has_idaq || rs->has_sqb || rs->baq_pending || rs->idq_mode || rs->h_ai || rs->h_ad || rs->h_sq
        || !rs->sq32.empty() || !rs->stored_fl.empty()) {
        return LFQ_ERR_INVALID;
    }
    const int64_t n = rs->n, nb = rs->n_bases;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(readset_upload_wait(rs));               /* the gather and permute kernels read all of it */
    lfq_baq_reads br;
    memset(&br, 0, sizeof(br));
    br.n_reads = n;
    br.pos = rs->pos; br.cigar_off = rs->cigar_off; br.cigar = rs->cigar; br.seq_off = rs->seq_off;
    br.seq = rs->seq; br.qual = rs->qual; br.ref = rs->ref; br.ref_len = rs->ref_len;
    LfqReadsDev dv;
    memset(&dv, 0, sizeof(dv));
    if (n > 0) {
        readset_view(rs, &dv);
    }
    const lfq_viterbi_result *res = nullptr;
    LFQ_TRY(lfq_viterbi_run(c, &br, def_qual, &dv, &res));

    /* the new order: by new position, ties in input order */
    LfqReadsetOwned *own = new LfqReadsetOwned();
    std::unique_ptr<LfqReadsetOwned> own_guard(own);
    own->order.resize((size_t)n);
    for (int64_t r = 0; r < n; r++) {
        own->order[(size_t)r] = r;
    }
    std::stable_sort(own->order.begin(), own->order.end(), [&](int64_t a, int64_t b) { return res->pos[a] < res->pos[b]; });
    own->pos.resize((size_t)std::max<int64_t>(n, 1));
    own->cigar_off.resize((size_t)n + 1);
    own->seq_off.resize((size_t)n + 1);
    own->flags.resize((size_t)std::max<int64_t>(n, 1));
    if (rs->mapq) own->mapq.resize((size_t)std::max<int64_t>(n, 1));
    if (rs->reverse) own->reverse.resize((size_t)std::max<int64_t>(n, 1));
    own->cigar_off[0] = own->seq_off[0] = 0;
    std::vector<int64_t> old_start((size_t)std::max<int64_t>(n, 1));
    for (int64_t j = 0; j < n; j++) {
        const int64_t r = own->order[(size_t)j];
        own->pos[(size_t)j] = res->pos[r];
        own->cigar_off[(size_t)j + 1] = own->cigar_off[(size_t)j] + (res->cigar_off[r + 1] - res->cigar_off[r]);
        own->seq_off[(size_t)j + 1] = own->seq_off[(size_t)j] + (rs->seq_off[r + 1] - rs->seq_off[r]);
        own->flags[(size_t)j] = rs->fl[(size_t)r];
        if (rs->mapq) own->mapq[(size_t)j] = rs->mapq[r];
        if (rs->reverse) own->reverse[(size_t)j] = rs->reverse[r];
        old_start[(size_t)j] = rs->seq_off[r];
    }
    own->cigar.resize((size_t)own->cigar_off[(size_t)n] + 1);
    own->seq.resize((size_t)nb + 1);
    own->qual.resize((size_t)nb + 1);
    if (rs->h_bi) own->bi.resize((size_t)nb + 1);
    if (rs->h_bd) own->bd.resize((size_t)nb + 1);
    own->ref.assign(rs->ref, rs->ref + rs->ref_len);
    own->ref.push_back('\0');
    lfq_for_reads(n, [&](int64_t j0, int64_t j1, int) {
        for (int64_t j = j0; j < j1; j++) {
            const int64_t r = own->order[(size_t)j];
            const int64_t nc = res->cigar_off[r + 1] - res->cigar_off[r], len = rs->seq_off[r + 1] - rs->seq_off[r];
            const int64_t s_old = rs->seq_off[r], s_new = own->seq_off[(size_t)j];
            if (nc > 0) {
                memcpy(own->cigar.data() + own->cigar_off[(size_t)j], res->cigar + res->cigar_off[r], (size_t)nc * 4);
            }
            if (len > 0) {
                memcpy(own->seq.data() + s_new, rs->seq + s_old, (size_t)len);
                memcpy(own->qual.data() + s_new, rs->qual + s_old, (size_t)len);
                if (rs->h_bi) memcpy(own->bi.data() + s_new, rs->h_bi + s_old, (size_t)len);
                if (rs->h_bd) memcpy(own->bd.data() + s_new, rs->h_bd + s_old, (size_t)len);
            }
        }
    });

    lfq_pileup_reads pr;
    memset(&pr, 0, sizeof(pr));
    pr.n_reads = n;
    pr.pos = own->pos.data(); pr.cigar_off = own->cigar_off.data(); pr.cigar = own->cigar.data();
    pr.seq_off = own->seq_off.data(); pr.seq = own->seq.data(); pr.qual = own->qual.data();
    pr.mapq = rs->mapq ? own->mapq.data() : nullptr; pr.reverse = rs->reverse ? own->reverse.data() : nullptr;
    pr.ref = own->ref.data(); pr.ref_len = rs->ref_len;
    lfq_pileup_indel_tags tg;
    memset(&tg, 0, sizeof(tg));
    tg.bi = rs->h_bi ? own->bi.data() : nullptr;
    tg.bd = rs->h_bd ? own->bd.data() : nullptr;
    tg.tag_flags = own->flags.data();
    lfq_readset *ns = nullptr;
    LFQ_TRY(readset_create(c, &pr, &tg, &ns, true));
    ns->own = own_guard.release();
    int rc = readset_upload_wait(ns);               /* the new offsets are on the device */
    if (rc == LFQ_OK && n > 0 && nb > 0) {
        const uint8_t *src[4];
        uint8_t *dst[4];
        int na = 0;
        src[na] = rs->d_seq; dst[na++] = ns->d_seq;
        src[na] = rs->d_qual; dst[na++] = ns->d_qual;
        if (rs->h_bi) { src[na] = rs->d_bi; dst[na++] = ns->d_bi; }
        if (rs->h_bd) { src[na] = rs->d_bd; dst[na++] = ns->d_bd; }
        rc = lfq_viterbi_permute(c, n, nb, (const int64_t *)ns->d_soff, old_start.data(), na, src, dst);
    }
    if (rc != LFQ_OK) {
        lfq_readset_destroy(ns);
        return rc;
    }
    *out = ns;
    if (result_out) *result_out = res;
    if (order_out) *order_out = ns->own->order.data();
    return LFQ_OK;
}

/* What both BAM entries refuse of an lfq_bam_records before a device is touched (include/lofreq_amd.h): n_reads < 0, a null
 * per-read array, and per record decreasing offsets, a negative length or fewer bytes than its fixed part.  Each entry's own:
 * the decode needs `ref`, the encode refuses a record of more than max_record bytes. */
static int bam_records_check(const lfq_bam_records *recs, bool need_ref, int64_t max_record, const int64_t *data_end = nullptr)
{
    const int64_t n = recs->n_reads;
    if (n < 0 || (n > 0 && (!recs->data || !recs->data_off || !recs->pos || !recs->flag || !recs->mapq || !recs->l_qname
                            || !recs->n_cigar || !recs->l_qseq || (need_ref && !recs->ref)))) {
        return LFQ_ERR_INVALID;
    }
    for (int64_t r = 0; r < n; r++) {
        const int64_t o0 = recs->data_off[r], o1 = data_end ? data_end[r] : recs->data_off[r + 1], l = recs->l_qseq[r];
        if (o1 < o0 || o1 > recs->data_off[r + 1] || o1 - o0 > max_record || l < 0
            || o1 - o0 < (int64_t)recs->l_qname[r] + 4 * (int64_t)recs->n_cigar[r] + (l + 1) / 2 + l) {
            return LFQ_ERR_INVALID;
        }
    }
    return LFQ_OK;
}

/* the records of a checked lfq_bam_records as they go down: byte data_off[r] of recs->data lies at data_off[r] - data_off[0] +
 * first_shift of the device buffer.  (After hipSetDevice: lfq_is_pinned asks the runtime.) */
static LfqBamIn bam_records_in(const lfq_bam_records *recs)
{
    LfqBamIn in = {nullptr, 0, 0, true};
    if (recs->n_reads > 0) {
        in.data = recs->data + recs->data_off[0];
        in.data_bytes = recs->data_off[recs->n_reads] - recs->data_off[0];
        in.first_shift = (int)((uintptr_t)in.data & 15);
        in.pinned = lfq_is_pinned(in.data);
    }
    return in;
}

/* The read set of BAM records as they lie in memory (bam1_t.data): what lfq_region_add_read's loop and lfq_readset_create build
 * from them, with the per-base work -- nibbles -> base codes, qualities, the BI / BD strings found among the aux fields -- done
 * by the two launches of lfq_bamrec.hip.  The host reads per READ only: descriptor checks, prefix sums, the CIGAR words.  *out
 * owns its host arrays (LfqReadsetOwned); the per-base ones come back from the device into pinned memory.  Blocks. */
int lfq_readset_from_bam_ends(lfq_ctx *c, const lfq_bam_records *recs, const int64_t *data_end, unsigned read_tags, lfq_readset **out)
{
    if (out) *out = nullptr;
    if (!c || !recs || !out || (read_tags & ~(unsigned)(LFQ_BAM_READ_LB | LFQ_BAM_READ_IDAQ))) {
        return LFQ_ERR_INVALID;
    }
    LFQ_TRY(bam_records_check(recs, true, INT64_MAX, data_end));
    const int64_t n = recs->n_reads;
    std::unique_ptr<LfqReadsetOwned> own(new LfqReadsetOwned());
    own->cigar_off.resize((size_t)n + 1);
    own->seq_off.resize((size_t)n + 1);
    own->cigar_off[0] = own->seq_off[0] = 0;
    for (int64_t r = 0; r < n; r++) {
        own->cigar_off[(size_t)r + 1] = own->cigar_off[(size_t)r] + recs->n_cigar[r];
        own->seq_off[(size_t)r + 1] = own->seq_off[(size_t)r] + recs->l_qseq[r];
    }
    const int64_t nb = own->seq_off[(size_t)n];
    own->pos.resize((size_t)std::max<int64_t>(n, 1));
    own->mapq.resize((size_t)std::max<int64_t>(n, 1));
    own->reverse.resize((size_t)std::max<int64_t>(n, 1));
    own->flags.resize((size_t)std::max<int64_t>(n, 1));
    own->cigar.resize((size_t)own->cigar_off[(size_t)n] + 1);
    LFQ_TRY_HIP(hipSetDevice(c->device));
    const LfqBamIn in = bam_records_in(recs);
    lfq_bam_times_reset(c, n, nb, in.data_bytes);
    lfq_pileup_reads pr;
    memset(&pr, 0, sizeof(pr));
    pr.n_reads = n;
    pr.ref = recs->ref; pr.ref_len = recs->ref_len;
    if (n == 0) {
        lfq_readset *es = nullptr;
        LFQ_TRY(readset_create(c, &pr, nullptr, &es));
        es->own = own.release();
        *out = es;
        return LFQ_OK;
    }
    const int64_t first = recs->data_off[0];
    LfqPin<int64_t> desc(c, (size_t)(3 * n + 1));       /* seq_off[n + 1] | seq_src[n] | rec_end[n] */
    LFQ_PIN_OK(desc);
    memcpy(desc.data(), own->seq_off.data(), (size_t)(n + 1) * sizeof(int64_t));
    int64_t *seq_src = desc.data() + n + 1, *rec_end = seq_src + n;
    LfqReadsetOwned *o = own.get();
    lfq_for_reads(n, [&](int64_t r0, int64_t r1, int) {
        for (int64_t r = r0; r < r1; r++) {
            const int64_t at = recs->data_off[r] - first + recs->l_qname[r], nc = recs->n_cigar[r];
            o->pos[(size_t)r] = recs->pos[r];
            o->mapq[(size_t)r] = recs->mapq[r];
            o->reverse[(size_t)r] = (uint8_t)((recs->flag[r] >> 4) & 1);
            if (nc > 0) {
                memcpy(o->cigar.data() + o->cigar_off[(size_t)r], in.data + at, (size_t)nc * 4);
            }
            seq_src[r] = in.first_shift + at + 4 * nc;
            rec_end[r] = in.first_shift + (data_end ? data_end[r] : recs->data_off[r + 1]) - first;
        }
    });
    int any_bi = 0, any_bd = 0;
    std::vector<uint8_t> stored(read_tags ? (size_t)n : 0);
    LFQ_TRY(lfq_bam_aux(c, in, desc.data(), n, nb, own->flags.data(), &any_bi, &any_bd, read_tags, stored.data()));
    uint32_t any_stored = 0;
    for (uint8_t f : stored) {
        any_stored |= f;
    }
    /* the pinned landing area of the per-base arrays, from the context's cache; the host views of the read set point into it */
    const size_t stride = (size_t)lfq_al(nb + 16);
    own->pin_bases = (uint8_t *)rs_cache_take(c, LFQ_RSC_PINBASES, stride * (size_t)(2 + any_bi + any_bd), &own->pin_cap);
    if (!own->pin_bases) {
        return LFQ_ERR_NOMEM;
    }
    uint8_t *h_seq = own->pin_bases, *h_qual = h_seq + stride, *h_bi = any_bi ? h_qual + stride : nullptr,
            *h_bd = any_bd ? h_qual + stride * (size_t)(1 + any_bi) : nullptr;
    pr.pos = own->pos.data(); pr.cigar_off = own->cigar_off.data(); pr.cigar = own->cigar.data();
    pr.seq_off = own->seq_off.data(); pr.seq = h_seq; pr.qual = h_qual;
    pr.mapq = own->mapq.data(); pr.reverse = own->reverse.data();
    lfq_pileup_indel_tags tg;
    memset(&tg, 0, sizeof(tg));
    tg.bi = h_bi;
    tg.bd = h_bd;
    tg.tag_flags = own->flags.data();
    lfq_readset *ns = nullptr;
    int rc = readset_create(c, &pr, &tg, &ns, true);
    if (rc != LFQ_OK) {
        rs_cache_give(c, LFQ_RSC_PINBASES, own->pin_bases, own->pin_cap);
        return rc;
    }
    ns->own = own.release();
    rc = lfq_bam_bases(c, ns->d_seq, ns->d_qual, any_bi ? ns->d_bi : nullptr, any_bd ? ns->d_bd : nullptr, h_seq, h_qual, h_bi, h_bd);
    if (rc == LFQ_OK) {
        rc = readset_upload_wait(ns);               /* the per-read arrays are on the device */
    }
    if (rc == LFQ_OK && any_stored) {
        /* the strings the records carry, per base, beside the read set's arrays: the merge mask of a fill, then lb | ai | ad */
        const int64_t each = lfq_al(nb + 16);
        int64_t off = lfq_al(n);
        int64_t o_st[3];
        for (int t = 0; t < 3; t++) {
            o_st[t] = off;
            off += ((any_stored >> t) & 1u) ? each : 0;
        }
        ns->stored_blob = (uint8_t *)rs_cache_take(c, LFQ_RSC_STORED, (size_t)off, &ns->cap[LFQ_RSC_STORED]);
        if (!ns->stored_blob) {
            rc = LFQ_ERR_NOMEM;
        } else {
            ns->d_take = ns->stored_blob;
            for (int t = 0; t < 3; t++) {
                ns->d_st[t] = ((any_stored >> t) & 1u) ? ns->stored_blob + o_st[t] : nullptr;
            }
            ns->stored_fl.swap(stored);
            rc = lfq_bam_stored(c, ns->d_st);
        }
    }
    if (rc != LFQ_OK) {
        lfq_readset_destroy(ns);
        return rc;
    }
    *out = ns;
    return LFQ_OK;
}

int lfq_readset_create_from_bam(lfq_ctx *c, const lfq_bam_records *recs, lfq_readset **out)
{
    return lfq_readset_from_bam_ends(c, recs, nullptr, 0, out);
}

int lfq_readset_create_from_bam_tags(lfq_ctx *c, const lfq_bam_records *recs, unsigned read_tags, lfq_readset **out)
{
    return lfq_readset_from_bam_ends(c, recs, nullptr, read_tags, out);
}

int lfq_readset_fetch_stored_tags(lfq_ctx *c, lfq_readset *rs, uint8_t *lb_out, uint8_t *ai_out, uint8_t *ad_out,
                                  uint8_t *stored_flags_out)
{
    if (!c || !rs || rs->c != c) {
        return LFQ_ERR_INVALID;
    }
    if (rs->n == 0) {
        return LFQ_OK;
    }
    const size_t nb = (size_t)rs->n_bases;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    uint8_t *const dst[3] = {lb_out, ai_out, ad_out};
    for (int t = 0; t < 3; t++) {
        if (dst[t] && rs->d_st[t] && nb > 0) {
            LFQ_TRY_HIP(hipMemcpyAsync(dst[t], rs->d_st[t], nb, hipMemcpyDeviceToHost, c->stream));
        } else if (dst[t]) {
            memset(dst[t], 33, nb);
        }
    }
    LFQ_TRY_HIP(hipStreamSynchronize(c->stream));
    for (int64_t r = 0; stored_flags_out && r < rs->n; r++) {
        stored_flags_out[r] = rs->stored_fl.empty() ? 0 : rs->stored_fl[(size_t)r];
    }
    return LFQ_OK;
}

/* copies of the resident per-base inputs, from the DEVICE: bases (0..15), qualities, BI / BD bytes ('!' throughout for an array the
 * read set does not have) and per read bit 0 / 1 = has BI / BD; NULL = not wanted */
int lfq_readset_fetch_bases(lfq_ctx *c, lfq_readset *rs, uint8_t *seq_out, uint8_t *qual_out, uint8_t *bi_out, uint8_t *bd_out,
                            uint8_t *tag_flags_out)
{
    if (!c || !rs || rs->c != c || ((bi_out || bd_out || tag_flags_out) && rs->idq_mode)
        || (rs->n > 0 && ((seq_out && !rs->seq) || (qual_out && !rs->qual)))) {
        return LFQ_ERR_INVALID;                     /* (after lfq_readset_indelqual: lfq_readset_fetch_indelquals) */
    }
    if (rs->n == 0) {
        return LFQ_OK;
    }
    const size_t nb = (size_t)rs->n_bases;
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LFQ_TRY(readset_upload_wait(rs));
    const struct { uint8_t *dst; const uint8_t *src; bool have; } todo[4] = {
        {seq_out, rs->d_seq, true}, {qual_out, rs->d_qual, true}, {bi_out, rs->d_bi, rs->has_bi}, {bd_out, rs->d_bd, rs->has_bd}};
    for (const auto &x : todo) {
        if (x.dst && x.have && nb > 0) {
            LFQ_TRY_HIP(hipMemcpyAsync(x.dst, x.src, nb, hipMemcpyDeviceToHost, c->stream));
        } else if (x.dst) {
            memset(x.dst, 33, nb);
        }
    }
    LFQ_TRY_HIP(hipStreamSynchronize(c->stream));
    for (int64_t r = 0; tag_flags_out && r < rs->n; r++) {
        tag_flags_out[r] = (uint8_t)(rs->fl[(size_t)r] & 3u);
    }
    return LFQ_OK;
}

/* The inverse of lfq_readset_create_from_bam: the results of the read set's steps written into the bytes of the records the reads
 * came from, by the two launches of the encode in lfq_bamrec.hip.  The host reads per READ only: the checks, one descriptor per
 * read, pos and n_cigar of the result.  Blocks. */
int lfq_readset_encode_bam(lfq_ctx *c, lfq_readset *rs, const lfq_bam_records *recs, const int64_t *src, unsigned what,
                           const lfq_bam_encoded **out)
{
    if (out) *out = nullptr;
    if (!c || !rs || !recs || !out) {
        return LFQ_ERR_INVALID;
    }
    const unsigned known = LFQ_BAM_PUT_ALIGNMENT | LFQ_BAM_DROP_ALN_TAGS | LFQ_BAM_PUT_LB | LFQ_BAM_PUT_IDAQ | LFQ_BAM_KEEP_EXISTING
                           | LFQ_BAM_PUT_INDELQUAL;
    if (what == 0 || (what & ~known) || ((what & LFQ_BAM_KEEP_EXISTING) && !(what & (LFQ_BAM_PUT_LB | LFQ_BAM_PUT_IDAQ)))) {
        return LFQ_ERR_INVALID;
    }
    LFQ_TRY(bam_records_check(recs, false, INT32_MAX));     /* (the plan's ranges are int32 offsets in a record) */
    const int64_t n = recs->n_reads;
    if (rs->c != c || rs->n != n) {
        return LFQ_ERR_INVALID;
    }
    if (src) {
        std::vector<uint8_t> hit((size_t)n, 0);
        for (int64_t j = 0; j < n; j++) {
            if (src[j] < 0 || src[j] >= n || hit[(size_t)src[j]]) {
                return LFQ_ERR_INVALID;
            }
            hit[(size_t)src[j]] = 1;
        }
    }
    for (int64_t j = 0; j < n; j++) {
        if (recs->l_qseq[src ? src[j] : j] != rs->seq_off[j + 1] - rs->seq_off[j]) {
            return LFQ_ERR_INVALID;
        }
    }
    if (((what & LFQ_BAM_PUT_LB) && !rs->has_lb) || ((what & LFQ_BAM_PUT_IDAQ) && !rs->has_idaq)
        || ((what & LFQ_BAM_PUT_INDELQUAL) && !rs->idq_mode)
        || ((what & (LFQ_BAM_PUT_LB | LFQ_BAM_PUT_IDAQ)) && rs->filled)) {    /* (stored bytes are not what alnqual appends) */
        return LFQ_ERR_INVALID;
    }
    if (n == 0) {
        return lfq_bam_encode_empty(c, out);
    }
    LFQ_TRY_HIP(hipSetDevice(c->device));
    LfqBamEncIn in;
    memset(&in, 0, sizeof(in));
    in.recs = bam_records_in(recs);
    in.n = n;
    in.what = what;
    in.uniform = rs->idq_mode == LFQ_IDQ_UNIFORM;
    const int64_t first = recs->data_off[0];
    LfqPin<LfqBamRead> reads(c, (size_t)n);
    LFQ_PIN_OK(reads);
    std::vector<int64_t> src_v((size_t)n);
    std::vector<int32_t> pos_v((size_t)n);
    std::vector<uint32_t> nc_v((size_t)n);
    const bool put_aln = (what & LFQ_BAM_PUT_ALIGNMENT) != 0;
    LfqBamRead *rd = reads.data();
    lfq_for_reads(n, [&](int64_t j0, int64_t j1, int) {
        for (int64_t j = j0; j < j1; j++) {
            const int64_t s = src ? src[j] : j;
            LfqBamRead &R = rd[j];
            R.rec = in.recs.first_shift + recs->data_off[s] - first;
            R.end = in.recs.first_shift + recs->data_off[s + 1] - first;
            R.l_qseq = recs->l_qseq[s];
            R.n_cigar = recs->n_cigar[s];
            R.l_qname = recs->l_qname[s];
            R.flag = recs->flag[s];
            R.pad_ = 0;
            src_v[(size_t)j] = s;
            pos_v[(size_t)j] = put_aln ? rs->pos[j] : recs->pos[s];
            nc_v[(size_t)j] = put_aln ? (uint32_t)(rs->cigar_off[j + 1] - rs->cigar_off[j]) : recs->n_cigar[s];
        }
    });
    in.reads = rd;
    in.src = src_v.data();
    in.pos = pos_v.data();
    in.n_cigar = nc_v.data();
    /* what the kernels read of the read set is on the device and complete in the order of the context's stream */
    LFQ_TRY(readset_upload_wait(rs));
    if (rs->baq_pending) {
        LFQ_TRY_HIP(hipStreamWaitEvent(c->stream, rs->ev_baq, 0));
    }
    if ((what & LFQ_BAM_PUT_INDELQUAL) && rs->ev_idq) {
        LFQ_TRY_HIP(hipStreamWaitEvent(c->stream, rs->ev_idq, 0));
    }
    readset_view(rs, &in.rd);
    in.d_fl = rs->d_fl;
    in.d_lb = (what & LFQ_BAM_PUT_LB) ? rs->d_lb : nullptr;
    in.d_ai = (what & LFQ_BAM_PUT_IDAQ) ? rs->d_ai : nullptr;
    in.d_ad = (what & LFQ_BAM_PUT_IDAQ) ? rs->d_ad : nullptr;
    in.d_bi = (what & LFQ_BAM_PUT_INDELQUAL) ? rs->d_bi : nullptr;
    in.d_bd = (what & LFQ_BAM_PUT_INDELQUAL) ? rs->d_bd : nullptr;
    return lfq_bam_encode(c, &in, out);
}

}  // extern "C"
