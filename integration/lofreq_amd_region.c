/*
 * lofreq_amd_region.c -- see lofreq_amd_region.h.  Plain C against include/lofreq_amd.h.
 */
#include "lofreq_amd_region.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* The per-base arrays of a region (bases, qualities, BI, BD: 150 bytes per read each) live in pinned memory
 * (lfq_host_alloc): lfq_readset_create then queues their copies as DMA transfers and returns, the BAQ kernels wait for the
 * chunks they need on the device, and this thread goes on decoding the next region instead of sitting out the upload
 * (grow-only, so the cost of pinning is paid in the first regions). */
typedef struct { void *p; int64_t n, cap; size_t elt; int pinned; } rvec;

static int rv_reserve(rvec *v, int64_t more)
{
    if (v->n + more > v->cap) {
        int64_t c = v->cap ? v->cap : (v->pinned ? (int64_t)1 << 16 : 4096);
        void *q;
        while (v->n + more > c) {
            c *= 2;
        }
        if (v->pinned) {
            q = lfq_host_alloc((size_t)c * v->elt);
            if (q && v->n > 0) {
                memcpy(q, v->p, (size_t)v->n * v->elt);
            }
            if (q) {
                lfq_host_free(v->p);
            }
        } else {
            q = realloc(v->p, (size_t)c * v->elt);
        }
        if (!q) {
            return LFQ_ERR_NOMEM;
        }
        v->p = q;
        v->cap = c;
    }
    return LFQ_OK;
}

/* one lfq_region_add_bgzf call: where its blocks lie in the region's staging, and the part of their inflated bytes to scan */
typedef struct { int64_t comp_at, first, stop; } reg_chunk;

/* the reads of one region as the flat arrays lfq_readset_create takes; two of them, because the host arrays of region k
 * must stay as they are until region k is finished -- which happens while region k + 1 is being filled */
typedef struct {
    rvec pos, cig_off, cig, seq_off, seq, qual, mapq, rev, bi, bd, flags;
    /* lfq_region_add_record: the records as they lie in bam1_t.data (pinned: they go down by DMA) and their descriptors; pos,
     * mapq and flags above are shared with the array road */
    rvec rec, rec_off, rec_flag, rec_lqname, rec_ncig, rec_lqseq;
    /* lfq_region_add_bgzf: the compressed blocks of every chunk, one behind the other (pinned), the chunks, and -- filled by
     * lfq_region_end from the scans of the inflated bytes -- where each kept record ends; the descriptors above are shared with
     * the record road */
    rvec bgz, chunk, rec_end;
    int32_t bgz_tid;
    int fed_by;                     /* 0: no read yet, 1: lfq_region_add_read, 2: lfq_region_add_record, 3: lfq_region_add_bgzf */
    int64_t n, nb;
    int any_bi, any_bd;
    char *target;
    const char *ref;
    int64_t ref_len, beg, end;
    lfq_readset *rs;
    int started;
    /* the SNV tracks of the region: their first pass runs beside the BAQ kernels, the scatter pass is queued behind them
     * (lfq_readset_pileup_snv returns at once) */
    lfq_tracks t;
    int have_tracks;
    int64_t *col_pos_s, pos_cap;
} reg_buf;

struct lfq_region {
    lfq_ctx *ctx;
    lfq_conf *conf;
    lfq_region_opts o;
    lfq_region_emit_fn emit;
    void *user;
    reg_buf buf[2];
    int cur;                        /* buffer being filled */
    int open;                       /* lfq_region_begin called, lfq_region_end not yet */
    int64_t wo_idaq;
    int64_t max_depth;              /* lfq_region_set_max_depth; LFQ_NO_MAX_DEPTH by default */
    int max_depth_set;              /* lfq_region_set_max_depth was called: close takes the cap off the context again */
    const lfq_bed *bed;             /* lfq_region_set_bed; NULL = no targets (the default) */
    int bed_set;                    /* lfq_region_set_bed was called: close takes the targets off the context again */
    lfq_indelqual_conf idq;         /* lfq_region_set_indelqual; mode 0 = off (the default) */
    int vit_on, vit_def_qual;       /* lfq_region_set_viterbi; off by default */
    int reuse_tags;                 /* lfq_region_set_reuse_tags; 0 by default */
    lfq_region_emit_fn emit_summary; /* lfq_region_set_summary; NULL = off (the default) */
    void *summary_user;
    /* outputs, grown on demand */
    int64_t *col_pos_i, pos_cap;
    lfq_snv_record *srec;
    int64_t srec_cap;
    lfq_indel_record *irec;
    int64_t irec_cap;
};

void lfq_region_opts_init(lfq_region_opts *o)
{
    memset(o, 0, sizeof(*o));
    o->use_baq = 1;
    o->baq_extended = 1;
    o->use_idaq = 0;
    o->def_nm_q = -1;
    o->max_mq = 255;
    o->min_plp_bq = 3;
}

static void buf_init(reg_buf *b)
{
    memset(b, 0, sizeof(*b));
    b->pos.elt = sizeof(int32_t);
    b->cig_off.elt = b->seq_off.elt = sizeof(int64_t);
    b->cig.elt = sizeof(uint32_t);
    b->seq.elt = b->qual.elt = b->mapq.elt = b->rev.elt = b->bi.elt = b->bd.elt = b->flags.elt = 1;
    /* (the small per-read arrays too: a pageable source is staged by the runtime with copy kernels, 7 ms for the 50 MB of a
     * 2 M-read region, in front of everything else on the upload stream) */
    b->seq.pinned = b->qual.pinned = b->bi.pinned = b->bd.pinned = 1;
    b->pos.pinned = b->cig_off.pinned = b->cig.pinned = b->seq_off.pinned = b->mapq.pinned = b->rev.pinned = b->flags.pinned = 1;
    b->rec.elt = 1;
    b->rec.pinned = 1;
    b->rec_off.elt = sizeof(int64_t);
    b->rec_flag.elt = b->rec_lqname.elt = sizeof(uint16_t);
    b->rec_ncig.elt = sizeof(uint32_t);
    b->rec_lqseq.elt = sizeof(int32_t);
    b->bgz.elt = 1;
    b->bgz.pinned = 1;
    b->chunk.elt = sizeof(reg_chunk);
    b->rec_end.elt = sizeof(int64_t);
}

static void buf_free(reg_buf *b)
{
    rvec *all[] = {&b->pos, &b->cig_off, &b->cig, &b->seq_off, &b->seq, &b->qual, &b->mapq, &b->rev, &b->bi, &b->bd, &b->flags,
                   &b->rec, &b->rec_off, &b->rec_flag, &b->rec_lqname, &b->rec_ncig, &b->rec_lqseq, &b->bgz, &b->chunk, &b->rec_end};
    size_t i;
    for (i = 0; i < sizeof(all) / sizeof(all[0]); i++) {
        if (all[i]->pinned) {
            lfq_host_free(all[i]->p);
        } else {
            free(all[i]->p);
        }
    }
    free(b->target);
    free(b->col_pos_s);
}

int lfq_region_open(lfq_region **out, lfq_ctx *ctx, lfq_conf *conf, const lfq_region_opts *opts,
                    lfq_region_emit_fn emit, void *user)
{
    lfq_region *r;
    if (!out || !ctx || !conf || !opts || !emit) {
        return LFQ_ERR_INVALID;
    }
    if (lfq_abi_version() != LFQ_ABI_VERSION) {       /* lfq_conf and the read / column structs belong to the version */
        return LFQ_ERR_UNSUPPORTED;
    }
    r = (lfq_region *)calloc(1, sizeof(*r));
    if (!r) {
        return LFQ_ERR_NOMEM;
    }
    r->ctx = ctx;
    r->conf = conf;
    r->o = *opts;
    r->emit = emit;
    r->user = user;
    r->max_depth = LFQ_NO_MAX_DEPTH;
    buf_init(&r->buf[0]);
    buf_init(&r->buf[1]);
    /* the bulk of the indel columns (the quality arrays of the reads WITHOUT an event) stays on the device */
    lfq_set_indel_arrays_on_host(ctx, 0);
    *out = r;
    return LFQ_OK;
}

int lfq_region_set_max_depth(lfq_region *r, int64_t max_depth)
{
    int rc;
    if (!r || r->open || r->buf[0].started || r->buf[1].started) {
        return LFQ_ERR_INVALID;                 /* (a region in flight was started under the cap it had) */
    }
    rc = lfq_set_max_depth(r->ctx, max_depth);
    if (rc == LFQ_OK) {
        r->max_depth = max_depth;
        r->max_depth_set = 1;
    }
    return rc;
}

int lfq_region_set_bed(lfq_region *r, const lfq_bed *bed_or_null)
{
    int rc;
    if (!r || r->open || r->buf[0].started || r->buf[1].started) {
        return LFQ_ERR_INVALID;                 /* (a region in flight keeps the targets its read set was created under) */
    }
    rc = lfq_set_bed(r->ctx, NULL, NULL);       /* every region puts its own contig's table there (region_start) */
    if (rc == LFQ_OK) {
        r->bed = bed_or_null;
        r->bed_set = 1;
    }
    return rc;
}

int lfq_region_set_indelqual(lfq_region *r, const lfq_indelqual_conf *conf_or_null)
{
    if (!r || r->open || r->buf[0].started || r->buf[1].started
        || (conf_or_null && conf_or_null->mode != LFQ_IDQ_UNIFORM && conf_or_null->mode != LFQ_IDQ_DINDEL)) {
        return LFQ_ERR_INVALID;
    }
    memset(&r->idq, 0, sizeof(r->idq));
    if (conf_or_null) {
        r->idq = *conf_or_null;
    }
    return LFQ_OK;
}

int lfq_region_set_viterbi(lfq_region *r, int on, int def_qual)
{
    if (!r || r->open || r->buf[0].started || r->buf[1].started || (on && def_qual > 93) || (on && r->reuse_tags)) {
        return LFQ_ERR_INVALID;
    }
    r->vit_on = on != 0;
    r->vit_def_qual = def_qual;
    return LFQ_OK;
}

int lfq_region_set_reuse_tags(lfq_region *r, int mode)
{
    if (!r || r->open || r->buf[0].started || r->buf[1].started || mode < 0 || mode > 2 || (mode && r->vit_on)) {
        return LFQ_ERR_INVALID;
    }
    r->reuse_tags = mode;
    return LFQ_OK;
}

int lfq_region_set_summary(lfq_region *r, lfq_region_emit_fn emit_summary_line, void *user)
{
    if (!r || r->open || r->buf[0].started || r->buf[1].started) {
        return LFQ_ERR_INVALID;
    }
    r->emit_summary = emit_summary_line;
    r->summary_user = user;
    return LFQ_OK;
}

int lfq_region_begin(lfq_region *r, const char *target_name, const char *ref, int64_t ref_len, int64_t beg0, int64_t end0)
{
    reg_buf *b;
    if (!r || r->open || !target_name || !ref || ref_len <= 0 || beg0 < 0 || end0 < beg0) {
        return LFQ_ERR_INVALID;
    }
    b = &r->buf[r->cur];
    if (b->started) {
        return LFQ_ERR_INVALID;                 /* (cannot happen: lfq_region_end finishes the older region first) */
    }
    b->pos.n = b->cig.n = b->seq.n = b->qual.n = b->mapq.n = b->rev.n = b->bi.n = b->bd.n = b->flags.n = 0;
    b->cig_off.n = b->seq_off.n = 0;
    b->rec.n = b->rec_off.n = b->rec_flag.n = b->rec_lqname.n = b->rec_ncig.n = b->rec_lqseq.n = 0;
    b->bgz.n = b->chunk.n = b->rec_end.n = 0;
    b->fed_by = 0;
    b->n = b->nb = 0;
    b->any_bi = b->any_bd = 0;
    free(b->target);
    b->target = strdup(target_name);
    if (!b->target) {
        return LFQ_ERR_NOMEM;
    }
    b->ref = ref;
    b->ref_len = ref_len;
    b->beg = beg0;
    b->end = end0 > ref_len ? ref_len : end0;
    if (rv_reserve(&b->cig_off, 1) || rv_reserve(&b->seq_off, 1)) {
        return LFQ_ERR_NOMEM;
    }
    ((int64_t *)b->cig_off.p)[0] = 0;
    ((int64_t *)b->seq_off.p)[0] = 0;
    b->cig_off.n = b->seq_off.n = 1;
    r->open = 1;
    return LFQ_OK;
}

int lfq_region_add_read(lfq_region *r, int32_t pos, int flag, int mapq, int n_cigar, const uint32_t *cigar, int l_qseq,
                        const uint8_t *seq4, const uint8_t *qual, const char *bi, const char *bd)
{
    /* the 4-bit BAM base "=ACMGRSVTWYHKDBN" -> the library's base code: 0..3 = A, C, G, T and 4 = N as seq_nt16_int (htslib
     * hts.c) has them, 5..15 = the other letters in the order "=MRSVWYHKDB" (include/lofreq_amd.h: they behave like N except
     * where the reference compares or prints the LETTER of a read base) */
    static const uint8_t nt16_int[16] = {5, 0, 1, 6, 2, 7, 8, 9, 3, 10, 11, 12, 13, 14, 15, 4};
    reg_buf *b;
    int i;
    if (!r || !r->open || n_cigar < 0 || l_qseq < 0 || (n_cigar > 0 && !cigar) || (l_qseq > 0 && (!seq4 || !qual))
        || r->reuse_tags) {                     /* (lfq_region_set_reuse_tags: the tags come with records only) */
        return LFQ_ERR_INVALID;
    }
    /* plp.c:706-720 */
    if (mapq > r->o.max_mq) {
        mapq = r->o.max_mq;
    } else if (mapq < r->o.min_mq) {
        return 0;
    } else if (r->o.no_orphan && (flag & 1) && !(flag & 2)) {      /* BAM_FPAIRED without BAM_FPROPER_PAIR */
        return 0;
    }
    if (n_cigar == 0 || l_qseq == 0) {
        return 0;                               /* nothing the pileup could place */
    }
    b = &r->buf[r->cur];
    if (b->fed_by > 1) {
        return LFQ_ERR_INVALID;                 /* a region is fed by one of the three functions only */
    }
    b->fed_by = 1;
    if (rv_reserve(&b->pos, 1) || rv_reserve(&b->cig_off, 1) || rv_reserve(&b->seq_off, 1) || rv_reserve(&b->cig, n_cigar)
        || rv_reserve(&b->seq, l_qseq + 16) || rv_reserve(&b->qual, l_qseq + 16) || rv_reserve(&b->bi, l_qseq + 16)
        || rv_reserve(&b->bd, l_qseq + 16) || rv_reserve(&b->mapq, 1) || rv_reserve(&b->rev, 1) || rv_reserve(&b->flags, 1)) {
        return LFQ_ERR_NOMEM;
    }
    ((int32_t *)b->pos.p)[b->n] = pos;
    memcpy((uint32_t *)b->cig.p + b->cig.n, cigar, (size_t)n_cigar * 4);
    b->cig.n += n_cigar;
    ((int64_t *)b->cig_off.p)[b->n + 1] = b->cig.n;
    for (i = 0; i < l_qseq; i++) {
        ((uint8_t *)b->seq.p)[b->nb + i] = nt16_int[(seq4[i >> 1] >> ((~i & 1) << 2)) & 0xf];     /* bam_seqi */
    }
    memcpy((uint8_t *)b->qual.p + b->nb, qual, (size_t)l_qseq);
    /* BI / BD: the tag bytes as they are (quality + 33); a read without the tag counts as quality 0 (plp.c:1024-1060) */
    if (bi && (int)strlen(bi) >= l_qseq) {
        memcpy((uint8_t *)b->bi.p + b->nb, bi, (size_t)l_qseq);
        b->any_bi = 1;
    } else {
        memset((uint8_t *)b->bi.p + b->nb, 33, (size_t)l_qseq);
        bi = NULL;
    }
    if (bd && (int)strlen(bd) >= l_qseq) {
        memcpy((uint8_t *)b->bd.p + b->nb, bd, (size_t)l_qseq);
        b->any_bd = 1;
    } else {
        memset((uint8_t *)b->bd.p + b->nb, 33, (size_t)l_qseq);
        bd = NULL;
    }
    ((uint8_t *)b->flags.p)[b->n] = (uint8_t)((bi ? 1 : 0) | (bd ? 2 : 0));
    ((uint8_t *)b->mapq.p)[b->n] = (uint8_t)mapq;
    ((uint8_t *)b->rev.p)[b->n] = (flag & 16) ? 1 : 0;                  /* bam_is_rev */
    b->nb += l_qseq;
    b->seq.n = b->qual.n = b->bi.n = b->bd.n = b->nb;
    ((int64_t *)b->seq_off.p)[b->n + 1] = b->nb;
    b->n += 1;
    b->pos.n = b->mapq.n = b->rev.n = b->flags.n = b->n;
    b->cig_off.n = b->seq_off.n = b->n + 1;
    return 1;
}

int lfq_region_add_record(lfq_region *r, int32_t pos, int flag, int mapq, int l_qname, int n_cigar, int l_qseq,
                          const uint8_t *data, int l_data)
{
    reg_buf *b;
    if (!r || !r->open || l_qname < 0 || n_cigar < 0 || l_qseq < 0 || l_data < 0 || (l_data > 0 && !data)
        || (int64_t)l_data < (int64_t)l_qname + 4 * (int64_t)n_cigar + ((int64_t)l_qseq + 1) / 2 + l_qseq) {
        return LFQ_ERR_INVALID;
    }
    /* plp.c:706-720 */
    if (mapq > r->o.max_mq) {
        mapq = r->o.max_mq;
    } else if (mapq < r->o.min_mq) {
        return 0;
    } else if (r->o.no_orphan && (flag & 1) && !(flag & 2)) {      /* BAM_FPAIRED without BAM_FPROPER_PAIR */
        return 0;
    }
    if (n_cigar == 0 || l_qseq == 0) {
        return 0;                               /* nothing the pileup could place */
    }
    b = &r->buf[r->cur];
    if (b->fed_by == 1 || b->fed_by == 3) {
        return LFQ_ERR_INVALID;                 /* a region is fed by one of the three functions only */
    }
    b->fed_by = 2;
    if (rv_reserve(&b->pos, 1) || rv_reserve(&b->mapq, 1) || rv_reserve(&b->flags, 1) || rv_reserve(&b->rec, (int64_t)l_data + 16)
        || rv_reserve(&b->rec_off, 2) || rv_reserve(&b->rec_flag, 1) || rv_reserve(&b->rec_lqname, 1) || rv_reserve(&b->rec_ncig, 1)
        || rv_reserve(&b->rec_lqseq, 1)) {
        return LFQ_ERR_NOMEM;
    }
    /* the record as it lies: bases, qualities and aux fields are decoded on the device (lfq_readset_create_from_bam) */
    memcpy((uint8_t *)b->rec.p + b->rec.n, data, (size_t)l_data);
    ((int64_t *)b->rec_off.p)[b->n] = b->rec.n;
    b->rec.n += l_data;
    ((int64_t *)b->rec_off.p)[b->n + 1] = b->rec.n;
    ((int32_t *)b->pos.p)[b->n] = pos;
    ((uint8_t *)b->mapq.p)[b->n] = (uint8_t)mapq;
    ((uint16_t *)b->rec_flag.p)[b->n] = (uint16_t)flag;
    ((uint16_t *)b->rec_lqname.p)[b->n] = (uint16_t)l_qname;
    ((uint32_t *)b->rec_ncig.p)[b->n] = (uint32_t)n_cigar;
    ((int32_t *)b->rec_lqseq.p)[b->n] = l_qseq;
    b->nb += l_qseq;
    b->n += 1;
    b->pos.n = b->mapq.n = b->flags.n = b->rec_flag.n = b->rec_lqname.n = b->rec_ncig.n = b->rec_lqseq.n = b->n;
    b->rec_off.n = b->n + 1;
    return 1;
}

/* One chunk of an index query -- or the whole region -- as it lies in the file: n_bytes of whole BGZF blocks.  They are copied into
 * the region's pinned staging; lfq_region_end inflates, scans and decodes them on the device (lofreq_amd_region.h) */
int lfq_region_add_bgzf(lfq_region *r, int32_t tid, const uint8_t *comp, int64_t n_bytes, int64_t first, int64_t stop_or_neg)
{
    reg_buf *b;
    reg_chunk *c;
    if (!r || !r->open || n_bytes < 0 || (n_bytes > 0 && !comp) || first < 0 || (stop_or_neg >= 0 && stop_or_neg < first)) {
        return LFQ_ERR_INVALID;
    }
    b = &r->buf[r->cur];
    if (b->fed_by == 1 || b->fed_by == 2 || (b->chunk.n > 0 && b->bgz_tid != tid)) {
        return LFQ_ERR_INVALID;                 /* a region is fed by one of the three functions only, and lies on one contig */
    }
    b->fed_by = 3;
    b->bgz_tid = tid;
    if (rv_reserve(&b->bgz, n_bytes + 16) || rv_reserve(&b->chunk, 1)) {
        return LFQ_ERR_NOMEM;
    }
    if (n_bytes > 0) {
        memcpy((uint8_t *)b->bgz.p + b->bgz.n, comp, (size_t)n_bytes);
    }
    c = (reg_chunk *)b->chunk.p + b->chunk.n;
    c->comp_at = b->bgz.n;
    c->first = first;
    c->stop = stop_or_neg;
    b->bgz.n += n_bytes;
    b->chunk.n += 1;
    return LFQ_OK;
}

static int region_decoded_flags(lfq_region *r, reg_buf *b, int rc);

/* the read set of a region fed by lfq_region_add_record: decoded on the device */
static int region_readset_from_records(lfq_region *r, reg_buf *b)
{
    lfq_bam_records rc_;
    int rc;
    memset(&rc_, 0, sizeof(rc_));
    rc_.n_reads = b->n;
    rc_.data = (const uint8_t *)b->rec.p;
    rc_.data_off = (const int64_t *)b->rec_off.p;
    rc_.pos = (const int32_t *)b->pos.p;
    rc_.flag = (const uint16_t *)b->rec_flag.p;
    rc_.mapq = (const uint8_t *)b->mapq.p;
    rc_.l_qname = (const uint16_t *)b->rec_lqname.p;
    rc_.n_cigar = (const uint32_t *)b->rec_ncig.p;
    rc_.l_qseq = (const int32_t *)b->rec_lqseq.p;
    rc_.ref = b->ref;
    rc_.ref_len = b->ref_len;
    if (r->reuse_tags) {
        rc = lfq_readset_create_from_bam_tags(r->ctx, &rc_, LFQ_BAM_READ_LB | (r->o.use_idaq ? LFQ_BAM_READ_IDAQ : 0), &b->rs);
    } else {
        rc = lfq_readset_create_from_bam(r->ctx, &rc_, &b->rs);
    }
    return region_decoded_flags(r, b, rc);
}

/* the read set of a region fed by lfq_region_add_bgzf: the staged blocks inflated in one call, every chunk's part of the
 * inflated bytes scanned with the region's filters, the kept records of all chunks decoded from the device copy */
static int region_readset_from_bgzf(lfq_region *r, reg_buf *b)
{
    const lfq_bgzf_result *R = NULL;
    const reg_chunk *ch = (const reg_chunk *)b->chunk.p;
    lfq_bam_scan_opts so;
    lfq_bam_scan S;
    int64_t k, blk = 0, last_end = 0;
    int rc = lfq_bgzf_inflate(r->ctx, (const uint8_t *)b->bgz.p, b->bgz.n, &R);
    if (rc != LFQ_OK) {
        return rc;
    }
    lfq_bam_scan_opts_init(&so);
    so.tid = b->bgz_tid;
    so.beg = b->beg;
    so.end = b->end;
    so.min_mq = r->o.min_mq;
    so.max_mq = r->o.max_mq;
    so.no_orphan = r->o.no_orphan;
    b->n = b->nb = 0;
    for (k = 0; k < b->chunk.n; k++) {
        lfq_bam_scan *s = NULL;
        int64_t base, lim = R->n_bytes, first, stop, i, m;
        while (blk < R->n_blocks && R->comp_off[blk] < ch[k].comp_at) {
            blk++;
        }
        if (R->comp_off[blk] != ch[k].comp_at) {
            return LFQ_ERR_INVALID;             /* (a chunk is a whole number of blocks) */
        }
        base = R->data_off[blk];
        if (k + 1 < b->chunk.n) {
            int64_t nb_ = blk;
            while (nb_ < R->n_blocks && R->comp_off[nb_] < ch[k + 1].comp_at) {
                nb_++;
            }
            lim = R->data_off[nb_];
        }
        first = base + ch[k].first;
        stop = ch[k].stop < 0 ? lim : base + ch[k].stop;
        if (first > lim || stop > lim) {
            return LFQ_ERR_INVALID;
        }
        rc = lfq_bam_scan_records(R->data, first, stop, &so, &s);
        if (rc != LFQ_OK) {
            return rc;
        }
        m = s->recs.n_reads;
        if (rv_reserve(&b->pos, m) || rv_reserve(&b->mapq, m) || rv_reserve(&b->rec_off, m + 1) || rv_reserve(&b->rec_end, m)
            || rv_reserve(&b->rec_flag, m) || rv_reserve(&b->rec_lqname, m) || rv_reserve(&b->rec_ncig, m)
            || rv_reserve(&b->rec_lqseq, m)) {
            lfq_bam_scan_free(s);
            return LFQ_ERR_NOMEM;
        }
        for (i = 0; i < m; i++) {
            ((int64_t *)b->rec_off.p)[b->n + i] = s->recs.data_off[i];
            ((int64_t *)b->rec_end.p)[b->n + i] = s->data_end[i];
            ((int32_t *)b->pos.p)[b->n + i] = s->recs.pos[i];
            ((uint8_t *)b->mapq.p)[b->n + i] = s->recs.mapq[i];
            ((uint16_t *)b->rec_flag.p)[b->n + i] = s->recs.flag[i];
            ((uint16_t *)b->rec_lqname.p)[b->n + i] = s->recs.l_qname[i];
            ((uint32_t *)b->rec_ncig.p)[b->n + i] = s->recs.n_cigar[i];
            ((int32_t *)b->rec_lqseq.p)[b->n + i] = s->recs.l_qseq[i];
            b->nb += s->recs.l_qseq[i];
            last_end = s->data_end[i];
        }
        b->n += m;
        b->pos.n = b->mapq.n = b->rec_off.n = b->rec_end.n = b->rec_flag.n = b->rec_lqname.n = b->rec_ncig.n = b->rec_lqseq.n = b->n;
        lfq_bam_scan_free(s);
    }
    if (b->n == 0) {
        return LFQ_OK;
    }
    b->flags.n = 0;
    if (rv_reserve(&b->flags, b->n)) {
        return LFQ_ERR_NOMEM;
    }
    b->flags.n = b->n;
    ((int64_t *)b->rec_off.p)[b->n] = last_end;
    b->rec_off.n = b->n + 1;
    memset(&S, 0, sizeof(S));
    S.recs.n_reads = b->n;
    S.recs.data = R->data;
    S.recs.data_off = (const int64_t *)b->rec_off.p;
    S.recs.pos = (const int32_t *)b->pos.p;
    S.recs.flag = (const uint16_t *)b->rec_flag.p;
    S.recs.mapq = (const uint8_t *)b->mapq.p;
    S.recs.l_qname = (const uint16_t *)b->rec_lqname.p;
    S.recs.n_cigar = (const uint32_t *)b->rec_ncig.p;
    S.recs.l_qseq = (const int32_t *)b->rec_lqseq.p;
    S.recs.ref = b->ref;
    S.recs.ref_len = b->ref_len;
    S.data_end = (const int64_t *)b->rec_end.p;
    rc = lfq_readset_create_from_bam_scan(r->ctx, &S, r->reuse_tags ? LFQ_BAM_READ_LB | (r->o.use_idaq ? LFQ_BAM_READ_IDAQ : 0) : 0,
                                          &b->rs);
    return region_decoded_flags(r, b, rc);
}

/* which tags the reads of a decoded region came with is what the decode found */
static int region_decoded_flags(lfq_region *r, reg_buf *b, int rc)
{
    int64_t i;
    if (rc == LFQ_OK) {
        rc = lfq_readset_fetch_bases(r->ctx, b->rs, NULL, NULL, NULL, NULL, (uint8_t *)b->flags.p);
        if (rc != LFQ_OK) {
            lfq_readset_destroy(b->rs);
            b->rs = NULL;
        }
    }
    for (i = 0; rc == LFQ_OK && i < b->n; i++) {
        b->any_bi |= ((const uint8_t *)b->flags.p)[i] & 1;
        b->any_bd |= (((const uint8_t *)b->flags.p)[i] >> 1) & 1;
    }
    return rc;
}

/* region k: upload (asynchronous) + BAQ / IDAQ kernels (queued) + source quality */
static int region_start(lfq_region *r, reg_buf *b)
{
    lfq_pileup_reads rd;
    lfq_pileup_indel_tags tg;
    int rc = LFQ_OK;
    if (r->bed) {
        /* -l: the table of this region's contig, for the read set created below on any of the three roads (a read set takes the
         * context's targets when it is created; a contig the BED does not name gets an empty table: no read, no column) */
        rc = lfq_set_bed(r->ctx, r->bed, b->target);
        if (rc != LFQ_OK) {
            return rc;
        }
    }
    if (b->fed_by == 3) {
        rc = region_readset_from_bgzf(r, b);    /* (how many reads the region has is what the scan keeps) */
        if (rc != LFQ_OK) {
            return rc;
        }
    }
    if (b->n == 0) {
        b->started = 1;
        return LFQ_OK;
    }
    if (b->fed_by == 3) {
        /* decoded above */
    } else if (b->fed_by == 2) {
        rc = region_readset_from_records(r, b);
    } else {
        memset(&rd, 0, sizeof(rd));
        memset(&tg, 0, sizeof(tg));
        rd.n_reads = b->n;
        rd.pos = (const int32_t *)b->pos.p;
        rd.cigar_off = (const int64_t *)b->cig_off.p;
        rd.cigar = (const uint32_t *)b->cig.p;
        rd.seq_off = (const int64_t *)b->seq_off.p;
        rd.seq = (const uint8_t *)b->seq.p;
        rd.qual = (const uint8_t *)b->qual.p;
        rd.mapq = (const uint8_t *)b->mapq.p;
        rd.reverse = (const uint8_t *)b->rev.p;
        rd.ref = b->ref;
        rd.ref_len = b->ref_len;
        tg.bi = b->any_bi ? (const uint8_t *)b->bi.p : NULL;
        tg.bd = b->any_bd ? (const uint8_t *)b->bd.p : NULL;
        tg.tag_flags = (const uint8_t *)b->flags.p;
        rc = lfq_readset_create(r->ctx, &rd, &tg, &b->rs);
    }
    if (rc != LFQ_OK) {
        return rc;
    }
    if (r->vit_on) {
        /* `lofreq viterbi` + sort: a new read set that owns its host arrays takes the place of the uploaded one (blocks) */
        lfq_readset *realigned = NULL;
        rc = lfq_readset_viterbi(r->ctx, b->rs, r->vit_def_qual, &realigned, NULL, NULL);
        lfq_readset_destroy(b->rs);
        b->rs = realigned;
        if (rc != LFQ_OK) {
            return rc;
        }
    }
    if (r->o.use_baq || r->o.use_idaq) {                                /* plp.c:667-683 */
        if (r->reuse_tags && b->fed_by >= 2) {                        /* baq_flag 1, or 2 under -D (plp.c:676-678) */
            rc = lfq_readset_baq_fill(r->ctx, b->rs, r->o.baq_extended, r->o.use_idaq ? 1 : 0, r->reuse_tags == 2);
        } else {
            rc = lfq_readset_baq(r->ctx, b->rs, r->o.baq_extended, r->o.use_idaq ? 1 : 0);
        }
        if (rc != LFQ_OK) {
            /* the read set waits for its queued copies before it goes: the caller may refill this buffer's arrays */
            lfq_readset_destroy(b->rs);
            b->rs = NULL;
            return rc;
        }
    }
    if (r->idq.mode && !b->any_bi && !b->any_bd) {
        /* `lofreq indelqual` for a region whose reads came without BI / BD: computed on the device copy, beside the BAQ kernels */
        rc = lfq_readset_indelqual(r->ctx, b->rs, &r->idq);
        if (rc != LFQ_OK) {
            lfq_readset_destroy(b->rs);
            b->rs = NULL;
            return rc;
        }
    }
    if (r->o.use_sq) {                                                  /* plp.c:727-735; DEFAULT_MIN_BQ = 6 */
        rc = lfq_readset_source_qual(r->ctx, b->rs, r->o.def_nm_q, 6, NULL, NULL);
        if (rc != LFQ_OK) {
            lfq_readset_destroy(b->rs);
            b->rs = NULL;
            return rc;
        }
    }
    if (r->max_depth != LFQ_NO_MAX_DEPTH || r->bed) {
        /* which reads cap and targets keep: decided now, while this region's BAQ kernels run (both pileups share it) */
        rc = lfq_readset_kept_reads(r->ctx, b->rs, NULL, NULL);
        if (rc != LFQ_OK) {
            lfq_readset_destroy(b->rs);
            b->rs = NULL;
            return rc;
        }
    }
    b->have_tracks = 0;
    b->started = 1;
    return LFQ_OK;
}

/* the SNV tracks of the region; returns when the scatter pass is queued */
static int region_snv_tracks(lfq_region *r, reg_buf *b)
{
    const int64_t width = b->end - b->beg + 1;
    int rc;
    if (width > b->pos_cap) {
        int64_t *a = (int64_t *)realloc(b->col_pos_s, sizeof(int64_t) * (size_t)width);
        if (!a) {
            return LFQ_ERR_NOMEM;
        }
        b->col_pos_s = a;
        b->pos_cap = width;
    }
    rc = lfq_readset_pileup_snv(r->ctx, b->rs, b->beg, b->end, r->o.min_plp_bq, &b->t, b->col_pos_s);
    b->have_tracks = rc == LFQ_OK;
    return rc;
}

static int grow_out(lfq_region *r, int64_t width)
{
    if (width > r->pos_cap) {
        int64_t *c = (int64_t *)realloc(r->col_pos_i, sizeof(int64_t) * (size_t)width);
        if (!c) {
            return LFQ_ERR_NOMEM;
        }
        r->col_pos_i = c;
        r->pos_cap = width;
    }
    return LFQ_OK;
}

/* region k: both pileups, call_indels + call_snvs, output in column order, indels before SNVs within a column
 * (call_vars, lofreq_call.c:896 before :928) */
static int region_finish(lfq_region *r, reg_buf *b)
{
    const lfq_indel_columns *cols = NULL;
    lfq_tracks t;
    int64_t n_irec = 0, n_srec = 0, n_tests = 0, i = 0, k = 0;
    int rc = LFQ_OK;
    char line[768];

    if (!b->started) {
        return LFQ_OK;
    }
    b->started = 0;
    if (b->n == 0 || !b->rs) {
        return LFQ_OK;
    }
    rc = grow_out(r, b->end - b->beg + 1);
    if (rc == LFQ_OK && r->emit_summary) {
        /* plp_summary's header lines, before the region's calls (the indel pileup below is then this region's second) */
        const lfq_plp_summary *sm = NULL;
        const int cap = (int)strlen(b->target) + 1536;      /* a consensus key is below MAX_INDELSIZE = 256 (utils.h:38) */
        char *big = (char *)malloc((size_t)cap);
        int64_t c;
        if (!big) {
            rc = LFQ_ERR_NOMEM;
        } else {
            rc = lfq_readset_plp_summary(r->ctx, b->rs, b->beg, b->end, r->o.min_plp_bq, r->o.min_plp_idq, &sm);
        }
        for (c = 0; rc == LFQ_OK && c < sm->ncols; c++) {
            const int len = lfq_format_plp_summary(big, cap, b->target, sm, c);
            if (len < 0) {
                rc = len;
            } else {
                r->emit_summary(r->summary_user, big);
            }
        }
        free(big);
    }
    /* the consensus-indel gate of call_vars (:928-931) needs the indel fields even when no indel is called -- but
     * without BI / BD no event can win the consensus (its quality sum is 0, plp.c:1236-1270) */
    if (rc == LFQ_OK && (r->o.call_indels || b->any_bi || b->any_bd || r->idq.mode)) {
        rc = lfq_readset_pileup_indels(r->ctx, b->rs, b->beg, b->end, r->o.min_plp_idq, &cols, r->col_pos_i);
        if (rc == LFQ_OK && !r->o.only_indels) {
            rc = region_snv_tracks(r, b);       /* its scatter pass runs under the host part of the indel tests below */
        }
        if (rc == LFQ_OK && r->o.call_indels && cols && cols->ncols > 0) {
            const int64_t nev = cols->side[0].ev_off[cols->ncols] + cols->side[1].ev_off[cols->ncols];
            if (nev + 16 > r->irec_cap) {
                lfq_indel_record *q = (lfq_indel_record *)realloc(r->irec, sizeof(lfq_indel_record) * (size_t)(nev + 16));
                if (!q) {
                    rc = LFQ_ERR_NOMEM;
                } else {
                    r->irec = q;
                    r->irec_cap = nev + 16;
                }
            }
            if (rc == LFQ_OK) {
                rc = lfq_call_indels_batch(r->ctx, r->conf, cols, r->irec, r->irec_cap, &n_irec, &n_tests);
            }
        }
    }
    if (rc == LFQ_OK && !r->o.only_indels && !b->have_tracks) {
        rc = region_snv_tracks(r, b);           /* (no indel pileup ran) */
    }
    if (rc == LFQ_OK && b->have_tracks) {
        t = b->t;
        if (cols && cols->cons_indel && t.ncols > 0) {
            /* both pileups cover [beg, end]: another column count is an internal error, and going on would emit SNVs
             * at columns whose consensus is an indel (lofreq_call.c:928-931) */
            rc = cols->ncols == t.ncols ? lfq_pileup_skip_snv_columns(r->ctx, cols->cons_indel, cols->ncols) : LFQ_ERR_INVALID;
        }
        if (rc == LFQ_OK && t.ncols > 0) {
            if (3 * t.ncols > r->srec_cap) {
                lfq_snv_record *q = (lfq_snv_record *)realloc(r->srec, sizeof(lfq_snv_record) * (size_t)(3 * t.ncols));
                if (!q) {
                    rc = LFQ_ERR_NOMEM;
                } else {
                    r->srec = q;
                    r->srec_cap = 3 * t.ncols;
                }
            }
            if (rc == LFQ_OK) {
                rc = lfq_call_snvs_batch(r->ctx, r->conf, &t, /*tracks_on_device=*/1, r->srec, r->srec_cap, &n_srec, NULL, NULL);
            }
        }
    }
    while (rc == LFQ_OK && (i < n_srec || k < n_irec)) {
        const int64_t p_snv = i < n_srec ? b->col_pos_s[r->srec[i].col] : INT64_MAX;
        const int64_t p_ind = k < n_irec ? r->col_pos_i[r->irec[k].col] : INT64_MAX;
        if (p_ind <= p_snv) {
            /* ins_to_str / del_to_str (lofreq_call.c:255-303): REF / ALT of an indel event */
            const lfq_indel_record *e = &r->irec[k++];
            const lfq_indel_side *sd = &cols->side[e->side];
            const int64_t kl = sd->key_off[e->event + 1] - sd->key_off[e->event];
            const int64_t r0 = sd->rd_off[e->event], r1 = sd->rd_off[e->event + 1];
            char *ref = (char *)malloc((size_t)kl + 2), *alt = (char *)malloc((size_t)kl + 2);
            char *big = (char *)malloc((size_t)kl * 2 + 1024);
            int64_t q, has_aq = 0, c0, c1;
            int s;
            if (!ref || !alt || !big) {
                free(ref); free(alt); free(big);
                rc = LFQ_ERR_NOMEM;
                break;
            }
            ref[0] = alt[0] = (char)cols->ref_base[e->col];
            memcpy((e->side == 0 ? alt : ref) + 1, sd->key_chars + sd->key_off[e->event], (size_t)kl);
            (e->side == 0 ? alt : ref)[kl + 1] = 0;
            (e->side == 0 ? ref : alt)[1] = 0;
            lfq_format_indel_record(big, (int)(kl * 2 + 1024), b->target, p_ind, ref, alt, e->qual, e->dp, e->af, e->sb,
                                    e->ref_fw, e->ref_rv, e->alt_fw, e->alt_rv, e->hrun, NULL);
            r->emit(r->user, big);
            /* report_var: an indel call in a column where no read carried an alignment quality (has_indel_aqs, plp.c:1076, 1121) */
            for (s = 0; s < 2 && !has_aq; s++) {
                c0 = cols->side[s].rd_off[cols->side[s].ev_off[e->col]];
                c1 = cols->side[s].rd_off[cols->side[s].ev_off[e->col + 1]];
                for (q = c0; q < c1; q++) {
                    if (cols->side[s].rd_aq[q] >= 0) {
                        has_aq = 1;
                        break;
                    }
                }
            }
            (void)r0; (void)r1;
            if (!has_aq) {
                r->wo_idaq += 1;
            }
            free(ref); free(alt); free(big);
        } else {
            lfq_format_snv_record(line, (int)sizeof(line), b->target, p_snv, &r->srec[i], NULL);
            r->emit(r->user, line);
            i++;
        }
    }
    lfq_readset_destroy(b->rs);
    b->rs = NULL;
    return rc;
}

int lfq_region_end(lfq_region *r)
{
    reg_buf *mine, *prev;
    int rc;
    if (!r || !r->open) {
        return LFQ_ERR_INVALID;
    }
    r->open = 0;
    mine = &r->buf[r->cur];
    prev = &r->buf[r->cur ^ 1];
    /* the region before this one: its BAQ kernels ran while this one's reads were decoded */
    rc = region_finish(r, prev);
    if (rc != LFQ_OK) {
        return rc;
    }
    rc = region_start(r, mine);
    r->cur ^= 1;
    return rc;
}

int lfq_region_close(lfq_region *r, int64_t *wo_idaq)
{
    int rc;
    if (!r) {
        return LFQ_ERR_INVALID;
    }
    rc = region_finish(r, &r->buf[r->cur]);             /* the older one, if it is still pending */
    if (rc == LFQ_OK) {
        rc = region_finish(r, &r->buf[r->cur ^ 1]);
    }
    if (wo_idaq) {
        *wo_idaq = r->wo_idaq;
    }
    if (r->buf[0].rs) lfq_readset_destroy(r->buf[0].rs);
    if (r->buf[1].rs) lfq_readset_destroy(r->buf[1].rs);
    lfq_set_indel_arrays_on_host(r->ctx, 1);
    if (r->max_depth_set) {
        lfq_set_max_depth(r->ctx, LFQ_NO_MAX_DEPTH);
    }
    if (r->bed_set) {
        lfq_set_bed(r->ctx, NULL, NULL);
    }
    buf_free(&r->buf[0]);
    buf_free(&r->buf[1]);
    free(r->col_pos_i);
    free(r->srec);
    free(r->irec);
    free(r);
    return rc;
}
