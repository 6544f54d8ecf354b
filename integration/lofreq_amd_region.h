/*
 * lofreq_amd_region.h -- the READ-level binding: a region worker of `lofreq call` that hands the reads of a region to the
 * GPU once and gets VCF records back.
 *
 * What it replaces in the reference, per region (`lofreq call -r chr:beg-end`, or one bin of call-parallel):
 *     mplp_func's per-read work            plp.c:667-683 (BAQ / IDAQ: bam_prob_realn_core_ext), :727-735 (source quality)
 *     bam_mplp_auto + compile_plp_col      plp.c:1406-1447, 797-1288 (the pileup and the column builder)
 *     call_vars per column                 lofreq_call.c:887-935 (call_indels, call_snvs, report_var)
 * What stays with htslib on the CPU: opening the BAM, the index query, decompressing records into bam1_t, the read-level
 * filters of mplp_func (plp.c:608-620: unmapped / secondary / QC-fail / duplicate).  Its BED overlap (-l, plp.c:625-629) and the
 * column rule of plp.c:1412 are the device's once lfq_region_set_bed is called.  Unpacking a record's bases,
 * qualities and BI / BD tags is the device's with lfq_region_add_record, the caller's thread's with lfq_region_add_read; with
 * lfq_region_add_bgzf the decompression, the record iteration and those filters leave htslib too.  The column callback
 * (integration/lofreq_amd_shim.c) keeps working for everything that wants plp_col_t; this path is for `lofreq call`
 * itself, whose end-to-end time was the CPU pileup + BAQ once the per-column statistics ran on the GPU.
 *
 * This file needs include/lofreq_amd.h only (no htslib, no LoFreq headers): the caller hands in the fields of a BAM
 * record as they lie in bam1_t (see INTEGRATION.md 9 for the ten lines of htslib macros that do it, and for the
 * plp.c hunk).  Records come back as VCF lines through a callback, FILTER '.', exactly what report_var writes to
 * conf->vcf_out; conf's Bonferroni factors and test counters are advanced as the per-column loop advances them, so
 * main_call's epilogue (lofreq_call.c:1506-1564) runs unchanged.
 *
 * Pipeline: lfq_region_end(k) queues region k's upload and BAQ kernels and returns; the pileups, the calls and the
 * output of region k happen inside lfq_region_end(k + 1) (or lfq_region_close), i.e. the CPU decodes the reads of
 * region k + 1 while the GPU works on region k.  Output order = region order.
 */
#ifndef LOFREQ_AMD_REGION_H
#define LOFREQ_AMD_REGION_H

#include "lofreq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lfq_region_opts {
    int use_baq;            /* MPLP_BAQ (plp.h:44)            -- lofreq call default: on */
    int baq_extended;       /* MPLP_EXT_BAQ                   -- on */
    int use_idaq;           /* MPLP_IDAQ                      -- on with --call-indels */
    int use_sq;             /* MPLP_USE_SQ (-s)               -- off */
    int def_nm_q;           /* mplp_conf_t.def_nm_q (-T)      -- -1 */
    int call_indels;        /* --call-indels */
    int only_indels;        /* --only-indels */
    int min_mq, max_mq;     /* mplp_conf_t.min_mq / max_mq (plp.c:706-710): 0 / 255 */
    int min_plp_bq;         /* mplp_conf_t.min_plp_bq: 3 */
    int min_plp_idq;        /* mplp_conf_t.min_plp_idq: 0 */
    int no_orphan;          /* MPLP_NO_ORPHAN (plp.c:717): paired reads that are not a proper pair are dropped */
} lfq_region_opts;

void lfq_region_opts_init(lfq_region_opts *o);      /* the defaults of `lofreq call` (lofreq_call.c:1030-1066) */

typedef void (*lfq_region_emit_fn)(void *user, const char *vcf_line);
typedef struct lfq_region lfq_region;

/* ctx: the worker's context (lfq_create on lfq_pick_device()); conf: the caller's, advanced by every region */
int lfq_region_open(lfq_region **out, lfq_ctx *ctx, lfq_conf *conf, const lfq_region_opts *opts,
                    lfq_region_emit_fn emit, void *user);
/* -d / --max-depth (mplp_conf_t.max_depth): the cap of bam_mplp_set_maxcnt (plp.c:1391-1392) on the reads of every region
 * after this call; see lfq_set_max_depth.  Call it after lfq_region_open and before the first lfq_region_begin (a region in
 * flight keeps the cap it was started with: LFQ_ERR_INVALID).  Default: LFQ_NO_MAX_DEPTH, no cap.  It is not a field of
 * lfq_region_opts, whose size callers rely on.  The cap is the context's (lfq_set_max_depth) while the binding is open, and
 * lfq_region_close takes it off again (LFQ_NO_MAX_DEPTH) if this call set it.  A negative `lofreq call -d` keeps only the first
 * read of each start position in htslib, which is max_depth = 0 here: map it, do not pass -1 through. */
int lfq_region_set_max_depth(lfq_region *r, int64_t max_depth);
/* -l / --bed: the targets (lfq_bed_parse, include/lofreq_amd.h) of every region after this call, on all three feeding roads.  Each
 * region takes the table of its target_name (lfq_set_bed; a name the BED does not hold: no read, no column): a read that overlaps
 * no interval is dropped in front of BAQ and of the -d cap (plp.c:625-629), a column outside every interval is not tested and
 * takes no Bonferroni step (plp.c:1412).  The caller does NOT filter reads by the BED itself any more.  `bed` stays the caller's
 * and must outlive the binding; NULL switches it off.  Same calling rule as lfq_region_set_max_depth; lfq_region_close takes the
 * targets off the context again if this call set them. */
int lfq_region_set_bed(lfq_region *r, const lfq_bed *bed_or_null);
/* `lofreq indelqual` inside the binding (opt-in; default off): the reads of a region in which NO read came with a BI or BD tag
 * (bi == bd == NULL in lfq_region_add_read) get their indel qualities from lfq_readset_indelqual, between the BAQ step and the
 * indel pileup -- conf->mode LFQ_IDQ_DINDEL (`--dindel`, from the region's contig) or LFQ_IDQ_UNIFORM (`-u ins_qual,del_qual`).
 * A region with tagged reads is taken as it is.  NULL switches it off again.  Same calling rule as lfq_region_set_max_depth:
 * after lfq_region_open, before the first lfq_region_begin.  Not a field of lfq_region_opts, whose size callers rely on.
 * Dindel mode fails a region (LFQ_ERR_INVALID from lfq_region_end) whose reads hold an N or P operation, as the command does. */
int lfq_region_set_indelqual(lfq_region *r, const lfq_indelqual_conf *conf_or_null);
/* `lofreq viterbi` inside the binding (opt-in; default off): with on != 0, lfq_region_end creates the region's read set, realigns
 * it with lfq_readset_viterbi(def_qual: -q / --defqual, negative = the read's median quality), destroys the first read set and goes
 * on -- BAQ, indelqual, pileups, calls -- with the new one, whose reads are sorted by their new positions: the binding replaces
 * the `samtools sort` between `lofreq viterbi` and the next step.  lfq_region_end then BLOCKS for the realignment of the region
 * it starts (the traced states come back to the host) instead of returning when the BAQ kernels are queued.
 * Region edges: the reads handed in for a region are realigned as if `lofreq viterbi` had run on exactly those reads; a read
 * that the realignment moves across a region's edge stays in the region it was handed in for, and reads handed in out of position
 * order are accepted.  BI / BD tags handed in with the reads are carried along as they are.  def_qual above 93 is
 * LFQ_ERR_INVALID, as is a read with a quality above 93 that would be realigned (from lfq_region_end).  Same calling rule as
 * lfq_region_set_indelqual: after lfq_region_open, before the first lfq_region_begin.  Not a field of lfq_region_opts. */
int lfq_region_set_viterbi(lfq_region *r, int on, int def_qual);
/* The lb / ai / ad tags the records already carry (opt-in; default mode 0), for regions fed by lfq_region_add_record:
 *   0   every read's alignment qualities are recomputed, whatever tags its record has (the behaviour without this call);
 *   1   `lofreq call`'s default: the first lb field of a record -- and, with use_idaq, its first ai and ad field -- is kept, and the
 *       HMM runs only for the reads that lack one (lfq_readset_create_from_bam_tags + lfq_readset_baq_fill);
 *   2   `lofreq call -D`: as 1, but a stored lb is recomputed; stored ai / ad still win.
 * A BAM that went through `lofreq alnqual` gives the reference's VCF under mode 1 and launches no HMM kernel at all.  A record
 * whose first lb / ai / ad field is no Z string of at least l_qseq bytes fails its region (LFQ_ERR_INVALID from lfq_region_end).
 * Under a non-zero mode lfq_region_add_read is LFQ_ERR_INVALID (it has no tags to hand over), and so is the mode together with
 * lfq_region_set_viterbi (the tags belong to the alignment the records came with), from whichever call comes second.  Same calling
 * rule as lfq_region_set_indelqual.  Not a field of lfq_region_opts. */
int lfq_region_set_reuse_tags(lfq_region *r, int mode);
/* `lofreq call --plp-summary-only` / `lofreq plpsummary` beside the calls (opt-in; default off): with a callback, every region
 * also emits the header line of plp_summary (lofreq_call.c:445-459) of each of its columns, in column order, BEFORE the region's
 * VCF lines -- one lfq_readset_plp_summary call per region, which runs the indel pileup of the region whether or not indels are
 * called.  The VCF lines and conf's counters are the same with and without it.  NULL switches it off again: such a run makes the
 * launches it made before this function existed.  Same calling rule as lfq_region_set_max_depth: after lfq_region_open, before
 * the first lfq_region_begin.  Not a field of lfq_region_opts. */
int lfq_region_set_summary(lfq_region *r, lfq_region_emit_fn emit_summary_line_or_null, void *user);
/* `ref`: the contig, upper-cased (plp.c:652), valid until the NEXT lfq_region_end / lfq_region_close has returned */
int lfq_region_begin(lfq_region *r, const char *target_name, const char *ref, int64_t ref_len, int64_t beg0, int64_t end0);
/* one BAM record that passed the flag filters of plp.c:608-632, in file order (position-sorted).  The fields are
 * bam1_t's: core.pos, core.flag, core.qual, core.n_cigar + bam_get_cigar, core.l_qseq + bam_get_seq (4-bit packed,
 * two bases per byte) + bam_get_qual; bi / bd: the Z strings of the BI / BD tags (bam_aux_get(...) + 1) or NULL.
 * Applies min_mq / max_mq / no_orphan itself (plp.c:706-720).  Returns 1 if the read was taken, 0 if filtered. */
int lfq_region_add_read(lfq_region *r, int32_t pos, int flag, int mapq, int n_cigar, const uint32_t *cigar, int l_qseq,
                        const uint8_t *seq4, const uint8_t *qual, const char *bi_or_null, const char *bd_or_null);
/* The same record handed over AS IT LIES in bam1_t: core.pos, core.flag, core.qual, core.l_qname, core.n_cigar, core.l_qseq,
 * b->data, b->l_data.  No bam_aux_get, no per-base loop on this thread: the record is copied into a pinned staging buffer and
 * lfq_region_end decodes the region's records on the device (lfq_readset_create_from_bam) -- bases, qualities, and BI / BD from the
 * first Z field of that tag with at least l_qseq bytes, exactly what lfq_region_add_read makes of bam_aux_get(...) + 1.  Same
 * filters and return values as lfq_region_add_read; LFQ_ERR_INVALID for a record shorter than its fields.  A region is fed by ONE
 * of the two functions: mixing them within a region is LFQ_ERR_INVALID.  A malformed aux field fails the region
 * (LFQ_ERR_INVALID from lfq_region_end).  lfq_region_end blocks for the decode of the region it starts. */
int lfq_region_add_record(lfq_region *r, int32_t pos, int flag, int mapq, int l_qname, int n_cigar, int l_qseq,
                          const uint8_t *data, int l_data);
/* The region's reads as they lie IN THE FILE: n_bytes of whole BGZF blocks -- the compressed bytes between the two virtual offsets
 * of a chunk of the index query, with first = the low 16 bits of the chunk's begin offset (where its first record starts in the
 * inflated bytes of its first block) and stop_or_neg = where to stop in the chunk's inflated bytes, or negative for their end.
 * Once or several times per region, chunks in file order, all of contig tid.  No sam_itr_next, no inflate on this thread: the
 * blocks are copied into a pinned staging buffer, and lfq_region_end inflates them on the device (lfq_bgzf_inflate), scans every
 * chunk's records with the filters of plp.c:606-722 (lfq_bam_scan_records: refID == tid, the flag mask 4 | 256 | 512 | 1024, overlap
 * with the region's [beg0, end0), min_mq / max_mq / no_orphan of the options) and decodes the kept ones from the device copy
 * (lfq_readset_create_from_bam_scan) -- with lfq_region_set_reuse_tags as for lfq_region_add_record.  BED overlap is
 * lfq_region_set_bed's, as on the other roads; MPLP_ILLUMINA13 is not applied on this road.  VCF lines, counters and the return values of lfq_region_end are those of the same
 * records fed by lfq_region_add_record.  Returns LFQ_OK; mixing it with the other two functions within a region is
 * LFQ_ERR_INVALID.  A block that does not inflate, a malformed record chain or aux field fails the region (LFQ_ERR_INVALID from
 * lfq_region_end). */
int lfq_region_add_bgzf(lfq_region *r, int32_t tid, const uint8_t *comp, int64_t n_bytes, int64_t first, int64_t stop_or_neg);
int lfq_region_end(lfq_region *r);
/* finishes the last region; *indel_calls_wo_idaq_or_null: report_var's counter (lofreq_call.c:109-111) */
int lfq_region_close(lfq_region *r, int64_t *indel_calls_wo_idaq_or_null);

#ifdef __cplusplus
}
#endif
#endif
