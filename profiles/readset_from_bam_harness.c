/*
 * readset_from_bam_harness.c -- the two roads of profiles/readset_from_bam_rate.py in C, so that what is timed is the binding
 * and not an interpreter: BAM records (bam1_t.data) of one region through integration/lofreq_amd_region.c,
 *   road 0   what a caller of lfq_region_add_read does per record: two bam_aux_get walks (restated below: htslib is not needed
 *            to walk an aux block), the pointers into the record, lfq_region_add_read -- whose loop unpacks the bases;
 *   road 1   lfq_region_add_record: the record as it lies.
 * then lfq_region_end, which creates the read set (BAQ, source quality and indelqual are off: nothing else is started).
 * Compiled together with integration/lofreq_amd_region.c by the script.
 */
#include "lofreq_amd_region.h"

#include <string.h>
#include <time.h>

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

static void no_line(void *user, const char *line)
{
    (void)user; (void)line;
}

/* bam_aux_get: the value (type byte first) of the first field with `tag`, or NULL */
static const uint8_t *aux_get(const uint8_t *s, const uint8_t *end, const char *tag)
{
    while (s + 3 <= end) {
        const uint8_t *v = s + 2;
        const int hit = s[0] == (uint8_t)tag[0] && s[1] == (uint8_t)tag[1];
        size_t size;
        if (hit) {
            return v;
        }
        switch (*v) {
        case 'A': case 'c': case 'C': size = 1; break;
        case 's': case 'S': size = 2; break;
        case 'i': case 'I': case 'f': size = 4; break;
        case 'Z': case 'H': size = strlen((const char *)v + 1) + 1; break;
        case 'B': {
            const int es = (v[1] == 'c' || v[1] == 'C') ? 1 : (v[1] == 's' || v[1] == 'S') ? 2 : 4;
            uint32_t cnt;
            memcpy(&cnt, v + 2, 4);
            size = 5 + (size_t)es * cnt;
            break;
        }
        default: return NULL;
        }
        s = v + 1 + size;
    }
    return NULL;
}

/* reps + 1 passes (the first one warms the binding's pinned buffers up and is reported like the others: the caller drops it).
 * ms_add[i]: the add loop on this thread; ms_total[i]: from lfq_region_begin until lfq_region_end has returned -- with
 * LFQ_SYNC_UPLOAD=1 the array road's uploads have landed by then, and the record road blocks anyway. */
int lfq_prof_road(lfq_ctx *ctx, lfq_conf *conf, int road, int64_t n, const uint8_t *data, const int64_t *off, const int32_t *pos,
                  const uint16_t *flag, const uint8_t *mapq, int l_qname, int n_cigar, int l_qseq, const char *ref, int64_t ref_len,
                  int passes, double *ms_add, double *ms_total)
{
    lfq_region_opts o;
    lfq_region *r = NULL;
    int rc, i;
    lfq_region_opts_init(&o);
    o.use_baq = o.baq_extended = o.use_idaq = o.use_sq = o.call_indels = 0;
    o.only_indels = 1;
    rc = lfq_region_open(&r, ctx, conf, &o, no_line, NULL);
    for (i = 0; rc == LFQ_OK && i < passes; i++) {
        int64_t k;
        const double t0 = now_ms();
        double t1;
        rc = lfq_region_begin(r, "chr1", ref, ref_len, 0, ref_len);
        for (k = 0; rc == LFQ_OK && k < n; k++) {
            const uint8_t *d = data + off[k], *end = data + off[k + 1];
            int took;
            if (road == 0) {
                const uint8_t *cig = d + l_qname, *seq = cig + 4 * (size_t)n_cigar, *qual = seq + (l_qseq + 1) / 2, *aux = qual + l_qseq;
                const uint8_t *bi = aux_get(aux, end, "BI"), *bd = aux_get(aux, end, "BD");
                uint32_t cw[64];
                memcpy(cw, cig, 4 * (size_t)(n_cigar < 64 ? n_cigar : 64));         /* (bam_get_cigar is aligned in htslib) */
                took = lfq_region_add_read(r, pos[k], flag[k], mapq[k], n_cigar, cw, l_qseq, seq, qual,
                                           bi && *bi == 'Z' ? (const char *)bi + 1 : NULL, bd && *bd == 'Z' ? (const char *)bd + 1 : NULL);
            } else {
                took = lfq_region_add_record(r, pos[k], flag[k], mapq[k], l_qname, n_cigar, l_qseq, d, (int)(end - d));
            }
            if (took != 1) {
                rc = took < 0 ? took : LFQ_ERR_INVALID;
            }
        }
        t1 = now_ms();
        if (rc == LFQ_OK) {
            rc = lfq_region_end(r);
        }
        ms_add[i] = t1 - t0;
        ms_total[i] = now_ms() - t0;
        /* an empty region behind it: its lfq_region_end finishes the one above, outside the clock, and the next pass fills the
         * same one of the binding's two buffers again */
        if (rc == LFQ_OK) {
            rc = lfq_region_begin(r, "chr1", ref, ref_len, 0, ref_len);
        }
        if (rc == LFQ_OK) {
            rc = lfq_region_end(r);
        }
    }
    if (r) {
        const int rc2 = lfq_region_close(r, NULL);
        rc = rc == LFQ_OK ? rc2 : rc;
    }
    return rc;
}
