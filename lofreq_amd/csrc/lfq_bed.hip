/*
 * lfq_bed.hip -- the targets of `lofreq call -l` (include/lofreq_amd.h: lfq_bed_*, lfq_set_bed): the BED on the host, the table of one
 * name on the device, and the two kernels that apply lfq_bed.h's predicate there.
 *
 *   reads     plp.c:625-629: a read whose [pos, bam_endpos) overlaps no interval never reaches the pileup.  One lane per read: the end
 *             from its CIGAR words, one binary search in the table, one byte out.  The read set (lfq_readset.hip) brings the bytes
 *             back once: the BAQ launch lists and the -d rule are made on the host.
 *   columns   plp.c:1412: a column whose [pos, pos + 1) overlaps no interval is skipped.  One lane per position of the region, between
 *             the count pass and the column compaction: the coverage of a position outside every interval goes to 0, and a position
 *             without coverage is no column -- the rule the compaction (lfq_plp_compact_*) and the host half of the indel pileup
 *             already have.  The kept reads do cover such positions, the flanks of every target: the scatter kernels take "no
 *             column" (-1) from the compaction's position -> column table (lfq_pileup.hip).
 */
#include "lfq_ctx.h"

__global__ __launch_bounds__(256) void lfq_bed_keep_kernel(LfqBedTab tab, const int32_t *__restrict__ pos,
                                                           const int64_t *__restrict__ cigar_off, const uint32_t *__restrict__ cigar,
                                                           int64_t n, uint8_t *__restrict__ keep_out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) {
        return;
    }
    const int64_t co = cigar_off[r], p = pos[r];
    keep_out[r] = (uint8_t)lfq_bed_tab_overlap(tab, p, lfq_bed_endpos(p, cigar + co, cigar_off[r + 1] - co));
}

__global__ __launch_bounds__(256) void lfq_bed_mask_columns_kernel(LfqBedTab tab, int64_t begin, int64_t width, int32_t *__restrict__ cov,
                                                                   int32_t *__restrict__ nb)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= width || cov[p] <= 0) {
        return;
    }
    if (!lfq_bed_tab_overlap(tab, begin + p, begin + p + 1)) {
        cov[p] = 0;
        if (nb) {
            nb[p] = 0;
        }
    }
}

int lfq_launch_bed_keep(const LfqBedTab &tab, const int32_t *pos, const int64_t *cigar_off, const uint32_t *cigar, int64_t n,
                        uint8_t *keep_out, void *stream)
{
    if (n <= 0) {
        return LFQ_OK;
    }
    hipLaunchKernelGGL(lfq_bed_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab, pos, cigar_off,
                       cigar, n, keep_out);
    return hipGetLastError() == hipSuccess ? LFQ_OK : LFQ_ERR_HIP;
}

int lfq_launch_bed_mask_columns(const LfqBedTab &tab, int64_t begin, int64_t width, int32_t *cov, int32_t *nb_or_null, void *stream)
{
    if (width <= 0) {
        return LFQ_OK;
    }
    hipLaunchKernelGGL(lfq_bed_mask_columns_kernel, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab, begin,
                       width, cov, nb_or_null);
    return hipGetLastError() == hipSuccess ? LFQ_OK : LFQ_ERR_HIP;
}

void lfq_bed_dev_release(LfqBedDev *b)
{
    if (b && b->refs.fetch_sub(1) == 1) {
        if (b->d) (void)hipFree(b->d);
        delete b;
    }
}

extern "C" {

int lfq_bed_parse(const char *text, int64_t n_bytes, lfq_bed **bed_out, int64_t *bad_line)
{
    if (bad_line) {
        *bad_line = 0;
    }
    if (!bed_out || n_bytes < 0 || (n_bytes > 0 && !text)) {
        return LFQ_ERR_INVALID;
    }
    *bed_out = nullptr;
    lfq_bed *bed = new lfq_bed();
    if (!lfq_bed_parse_text(text, n_bytes, bed, bad_line)) {
        delete bed;
        return LFQ_ERR_INVALID;
    }
    *bed_out = bed;
    return LFQ_OK;
}

void lfq_bed_free(lfq_bed *bed) { delete bed; }

int64_t lfq_bed_n_names(const lfq_bed *bed) { return bed ? (int64_t)bed->names.size() : 0; }

const char *lfq_bed_name(const lfq_bed *bed, int64_t i)
{
    return bed && i >= 0 && i < (int64_t)bed->names.size() ? bed->names[(size_t)i].name.c_str() : nullptr;
}

int lfq_bed_intervals(const lfq_bed *bed, const char *name, const int32_t **beg_out, const int32_t **end_out, int64_t *n_out)
{
    if (!bed || !name || !beg_out || !end_out || !n_out) {
        return LFQ_ERR_INVALID;
    }
    const LfqBedName *T = bed->find(name);
    *beg_out = T && !T->beg.empty() ? T->beg.data() : nullptr;
    *end_out = T && !T->beg.empty() ? T->end.data() : nullptr;
    *n_out = T ? (int64_t)T->beg.size() : 0;
    return LFQ_OK;
}

int lfq_bed_overlap(const lfq_bed *bed, const char *name, int64_t beg, int64_t end)
{
    const LfqBedName *T = bed ? bed->find(name) : nullptr;
    return T ? lfq_bed_tab_overlap(T->tab(), beg, end) : 0;
}

int lfq_set_bed(lfq_ctx *c, const lfq_bed *bed, const char *name)
{
    if (!c || (bed && !name)) {
        return LFQ_ERR_INVALID;
    }
    LfqBedDev *nb = nullptr;
    if (bed) {
        LFQ_TRY_HIP(hipSetDevice(c->device));
        nb = new LfqBedDev();
        nb->refs.store(1);
        nb->d = nullptr;
        const LfqBedName *T = bed->find(name);
        if (T) {
            nb->host = *T;
        }
        nb->host.name = name;
        const int64_t n = (int64_t)nb->host.beg.size();
        if (n > 0) {
            /* (a blocking copy from the context's own vectors: the table is small and set once per contig) */
            if (hipMalloc((void **)&nb->d, (size_t)n * 8) != hipSuccess) {
                delete nb;
                return LFQ_ERR_NOMEM;
            }
            if (hipMemcpy(nb->d, nb->host.beg.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess
                || hipMemcpy(nb->d + n, nb->host.pmax.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) {
                lfq_bed_dev_release(nb);
                return LFQ_ERR_HIP;
            }
        }
        nb->tab = {nb->d, nb->d ? nb->d + n : nullptr, n};
    }
    lfq_bed_dev_release(c->bed);
    c->bed = nb;
    return LFQ_OK;
}

}
