/*
 * lofreq_amd.h -- C ABI of the MI355X-native LoFreq per-column SNV calling path.
 *
 * This is the drop-in boundary for the path
 *     plp_to_errprobs -> qsort -> snpcaller/poissbin/pruned_calc_prob_dist -> Bonferroni emit test
 * of `lofreq call` (reference: src/lofreq/lofreq_call.c:735-879 call_snvs,
 * src/lofreq/snpcaller.c:346, 831, 1020, 1075).  Plain pointers and sizes only; no C++ or
 * torch types.  INTEGRATION.md shows the binding a LoFreq maintainer adds behind the
 * `void (*plp_proc_func)(const plp_col_t*, void*)` callback of mpileup() (plp.h:159-163).
 *
 * Layers:
 *   (1) lfq_snv_batch_device  -- kernels only, device pointers, asynchronous.  Replaces, for a
 *       batch of columns, the reference's inner numeric API plp_to_errprobs()+qsort()+snpcaller()
 *       (snpcaller.h:72-75, 97-102).
 *   (2) lfq_call_snvs_batch   -- the call_snvs() loop (lofreq_call.c:735-879) over a batch:
 *       runs (1), then does the 80-bit p-value conversion with the reference's errno/fenv clamp
 *       (snpcaller.c:1047-1059, 1169-1188), the running-Bonferroni emit test (lofreq_call.c:832),
 *       AF/DP4/HQA/QUAL (lofreq_call.c:835-863) and strand bias (lofreq_call.c:117-129) on the host,
 *       and returns one record per reported variant, in column order.
 *   (3) lfq_format_snv_record / lfq_filter_records / lfq_snvqual_thresh -- VCF text (vcf.c:469-497,
 *       608-629) and the final `lofreq filter` step that `lofreq call` runs on its own output
 *       (lofreq_call.c:1506-1538; lofreq_filter.c).
 *
 * All functions return 0 on success or a negative lfq_status.  Errors never fall back to a CPU
 * implementation: if no HIP device / kernel image is available the call fails.
 */
#ifndef LOFREQ_AMD_H
#define LOFREQ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: lfq_conf grew to 80 bytes (approx_threshold_n), lfq_dp_work gained n_approx_pruned, lfq_filter_records_ex.
 * A caller compiled against another version must not run: compare lfq_abi_version() with this value once, as the
 * bindings in integration/ and the Python loader do. */
/* 4: lfq_set_batch_gate, lfq_last_baq_times; lfq_call_snvs_collect refuses h_counts for a batch whose dense entries are sparse. */
/* 5: lfq_set_private_stream. */
/* 7: lfq_set_max_depth, lfq_readset_kept_reads. */
/* 8: lfq_viterbi_batch, lfq_last_viterbi_times. */
/* 9: lfq_indelqual_batch, lfq_readset_indelqual, lfq_readset_fetch_indelquals, lfq_last_indelqual_times. */
/* (10 still: lfq_readset_pileup_sites, lfq_readset_uniq, lfq_last_sites_times are new functions with new structs; no existing layout changed.) */
/* (10 still: lfq_readset_plp_summary, lfq_format_plp_summary, lfq_last_summary_times are new functions with new structs; no existing layout changed.) */
/* (10 still: lfq_plp_quals_from_tracks, lfq_format_plp_quals, lfq_format_plp_indel_quals, lfq_set_indel_arrays_all_columns, lfq_last_plp_quals_times are new functions with new structs; no existing layout changed.) */
/* (10 still: lfq_readset_create_from_bam, lfq_readset_fetch_bases, lfq_last_bam_decode_times are new functions with new structs; no existing layout changed.) */
/* (10 still: lfq_readset_create_from_bam_tags, lfq_readset_fetch_stored_tags, lfq_readset_baq_fill, lfq_last_baq_fill_stats likewise.) */
/* (10 still: lfq_readset_encode_bam, lfq_last_bam_encode_times are new functions with new structs; no existing layout changed.) */
/* (10 still: lfq_bgzf_inflate, lfq_last_bgzf_times, lfq_bam_scan_records and its helpers, lfq_readset_create_from_bgzf likewise.) */
/* (10 still: lfq_bgzf_deflate, lfq_last_bgzf_deflate_times, lfq_bam_frame_encoded, and the lfq_bam_index_* / lfq_bam_record_* functions are
 * new functions with new structs; no existing layout changed.) */
/* (10 still: lfq_bed_parse and the other lfq_bed_* functions, lfq_set_bed are new functions with a new opaque type; no existing layout changed.) */
/* (10 still: the lfq_fasta_* functions, lfq_last_fasta_times, lfq_checkref, lfq_bgzf_gzi_bytes, lfq_readset_ref_from_device are new functions with
 * new types; no existing layout changed.) */
#define LFQ_ABI_VERSION 10

typedef enum lfq_status {
    LFQ_OK = 0,
    LFQ_ERR_INVALID = -1,      /* bad argument */
    LFQ_ERR_NO_DEVICE = -2,    /* no HIP device or HIP runtime error */
    LFQ_ERR_NOMEM = -3,
    LFQ_ERR_CAPACITY = -4,     /* caller-provided output capacity too small */
    LFQ_ERR_UNSUPPORTED = -5,  /* option the reference rejects too (def_alt_jq == -1) */
    LFQ_ERR_HIP = -6
} lfq_status;

/* varcall_conf_t flag bits (defaults.h:71-76) */
#define LFQ_USE_BAQ 1
#define LFQ_USE_MQ 2
#define LFQ_USE_SQ 4
#define LFQ_USE_IDAQ 8

/* ---- packed column batch ------------------------------------------------------------------
 * Struct-of-arrays, one byte per observation per track, columns concatenated (CSR offsets).
 * Built from plp_col_t's per-nucleotide int_varray_t arrays (plp.h:88-91):
 *   nt   bits 0..2 = nt4 code (0..3 = A,C,G,T; 4 = N, skipped like snpcaller.c:386),
 *        bit 3 = read on reverse strand (feeds fw_counts/rv_counts, plp.c:1007-1011)
 *   bq   base quality, 0..93 (plp.c:937-953)
 *   baq  base alignment quality 0..93; 255 = missing (-1, plp.c:956-962).  NULL track = BAQ off.
 *   mq   mapping quality as in the BAM record, 0..255 (255 = NA is handled as snpcaller.c:451 does)
 *   sq   source quality 0..253; 254 = anything larger (source_qual's 49314: probability 0.0); 255 = missing (-1).
 *        NULL track = no source quality.
 * Track base pointers must be 16-byte aligned and readable up to the next multiple of 16 bytes
 * past col_off[ncols]; col_off itself may be arbitrary (columns need not be aligned).
 *
 * LFQ_TRACKS_NT_PACKED (flags): the nt track holds two observations per byte ((n_obs + 7) / 8 * 4 bytes).  What the device
 * pileup (lfq_pileup_snv_tracks / lfq_readset_pileup_snv) hands out by default, what the plp_proc_func shim
 * (integration/lofreq_amd_shim.c) builds as the columns arrive, and what lfq_pack_nt_track makes of a byte track.
 * Observations are taken in groups of 8 (by their index in the track); byte k (k = 0..3) of a group's 4 bytes
 * carries observation k in its low nibble and observation 4 + k in its high nibble -- the even / odd nibbles of a
 * dword then line up with the group's two bq dwords.  The count kernel, the dominant one and HBM-bound, reads
 * 1.5 instead of 2 bytes per observation.
 */
#define LFQ_TRACKS_NT_PACKED 1
#define LFQ_Q_MISSING 255

typedef struct lfq_tracks {
    const uint8_t *nt;
    const uint8_t *bq;
    const uint8_t *baq;        /* may be NULL */
    const uint8_t *mq;
    const uint8_t *sq;         /* may be NULL */
    const uint64_t *col_off;   /* ncols + 1 entries */
    const uint8_t *ref_base;   /* ncols ASCII reference bases (plp_col_t.ref_base); no alignment required (a count kernel reads the aligned
                                * 32-bit word around a column's byte: same page, never past a mapping) */
    const int32_t *coverage_plp; /* ncols, or NULL: = observation count (plp_col_t.coverage_plp) */
    const int32_t *num_bases;    /* ncols, or NULL: = observation count (plp_col_t.num_bases) */
    int64_t ncols;
    int64_t max_col_obs;         /* deepest column of the batch, or 0 = unknown (costs one sync) */
    int64_t flags;               /* LFQ_TRACKS_NT_PACKED or 0 */
} lfq_tracks;

/* the SNV-path fields of varcall_conf_t (snpcaller.h:38-63); defaults: lfq_conf_init */
typedef struct lfq_conf {
    int32_t min_bq, min_alt_bq, def_alt_bq;
    int32_t min_jq, min_alt_jq, def_alt_jq;
    int32_t bonf_dynamic;
    int32_t min_cov;
    int64_t bonf_subst;        /* running Bonferroni factor; mutated by lfq_call_snvs_batch */
    float sig;                 /* float, like the reference */
    int32_t flag;
    int64_t num_snv_tests;     /* the global of lofreq_call.c:84; mutated */
    int64_t bonf_indel;        /* running indel Bonferroni factor (snpcaller.h:52); mutated by the indel calls */
    int64_t num_indel_tests;   /* the global of lofreq_call.c:85; mutated */
    /* -t / --approx-threshold (snpcaller.h:62, snpcaller.c:1128-1142): a column or indel test with more error
     * probabilities than this is given up without the exact test when the Poisson tail with the same mean, times the
     * Bonferroni factor, exceeds sig.  <= 0 (default -1, snpcaller.c:650): off.  The reference needs libgsl for it (a
     * build without aborts, :1118-1125); here the definition gsl_cdf_poisson_P implements is evaluated -- parity
     * unpinned, see DESIGN.md.  It never adds a call and, as in the reference, does not change the Bonferroni counts. */
    int32_t approx_threshold_n;
    int32_t pad_;
} lfq_conf;

/* dense per-column output of the counting kernel == plp_to_errprobs()'s integer outputs
 * (snpcaller.c:346-498) plus the strand counts report_var() needs.  64 bytes. */
typedef struct lfq_col_counts {
    int32_t n_err_probs;       /* #probabilities the reference would hand to snpcaller */
    int32_t alt_counts[3];     /* filtered alt counts, alleles in A,C,G,T order minus ref */
    int32_t alt_raw_counts[3]; /* unfiltered alt counts (AF numerator, lofreq_call.c:835) */
    int32_t alt_fw[3];         /* forward-strand part of alt_raw_counts */
    int32_t ref_fw, ref_rv;    /* strand counts of the reference base */
    int32_t kmax;              /* max(alt_counts) = num_failures handed to poissbin */
    uint8_t tested;            /* column reaches the Bonferroni bump (lofreq_call.c:794-801) */
    uint8_t gated;             /* 1 = skipped by the ref-N / coverage gates (lofreq_call.c:747,754,930) */
    uint8_t pad_[2];
    int32_t median_ref_bq;     /* median reference-base BQ when def_alt_bq == -1, else -1 */
    int32_t coverage;          /* coverage_plp used for this column (DP / AF denominator) */
} lfq_col_counts;

/* status of one allele's p-value */
enum {
    LFQ_PV_NONE = 0,        /* count 0 or column pruned: reference returns LDBL_MAX */
    LFQ_PV_LOG = 1,         /* logp valid: pvalue = expl(logp) (+ the reference's clamp on expl) */
    LFQ_PV_LOG_FECLAMP = 2, /* logp valid but the reference's tail-sum exp() chain underflows
                               (snpcaller.c:1169-1188): pvalue clamps to LDBL_MIN / LDBL_MAX */
    LFQ_PV_UNDERFLOW = 3    /* p-value proven below the 80-bit range (logp = an upper bound < -12200):
                               the reference's expl() underflows and it reports LDBL_MIN */
};

/* sparse output: one record per column whose main allele survives the pruning test
 * P(X>=K)*bonf > sig (snpcaller.c:950, 1155).  128 bytes. */
typedef struct lfq_col_pvals {
    int64_t col;               /* column index within the batch */
    int64_t bonf;              /* running Bonferroni factor at this column */
    double logp[3];            /* natural-log p-values, same allele order as the counts */
    uint8_t status[3];
    uint8_t ref_base;          /* 'A','C','G','T': the column's reference base, so that the host needs no track */
    uint8_t pad_[4];
    lfq_col_counts counts;     /* copy of the dense entry, so the host needs nothing else */
    int32_t dp_rows;           /* DP rows processed (diagnostic) */
    int32_t pad2_;
    int64_t reserved_;
} lfq_col_pvals;

typedef struct lfq_batch_stats {
    int64_t n_tested;          /* columns that passed the gates with >= 1 filtered alt base */
    int64_t n_pvals;           /* records written to the sparse output */
    int64_t n_obs;             /* observations in the batch */
} lfq_batch_stats;

/* one reported SNV == the arguments of report_var() (lofreq_call.c:862-864) */
typedef struct lfq_snv_record {
    int64_t col;
    int32_t qual;              /* PROB_TO_PHREDQUAL(pvalue) */
    int32_t dp;                /* coverage_plp */
    int32_t alt_raw_count;     /* AF = alt_raw_count / (float) dp */
    int32_t sb;                /* strand-bias phred (INT_MAX special case included) */
    int32_t ref_fw, ref_rv, alt_fw, alt_rv;
    int32_t hqa;               /* filtered alt count */
    char ref, alt;
    uint8_t pad_[2];
    long double pvalue;
} lfq_snv_record;

typedef struct lfq_ctx lfq_ctx;

/* --- lifetime --- */
int lfq_abi_version(void);
const char *lfq_strerror(int status);
void lfq_conf_init(lfq_conf *conf);                 /* init_varcall_conf, snpcaller.c:627-651 */
int lfq_create(lfq_ctx **ctx, int device_ordinal);  /* one context per GPU / stream */
/* Which GPU a worker PROCESS takes.  The reference's parallel wrapper forks one `lofreq call -r <bin>` per worker
 * (lofreq2_call_pparallel.py:640-667); with this every such process lands on a GPU of its own without the wrapper
 * knowing about GPUs:  LFQ_DEVICE (an ordinal, taken literally)  >  LOCAL_RANK (torchrun-style launchers, modulo the
 * device count)  >  the first free worker slot k of the node (a lock file <LFQ_SLOT_DIR or /tmp>/lofreq_amd.<uid>.slot<k>
 * held for the life of the process: device k mod n, so W concurrent workers spread over the n GPUs and a slot is
 * reused when its worker exits)  >  getpid() mod n.  n_devices <= 0: ask the HIP runtime.  Returns the ordinal
 * (>= 0) for lfq_create, or a negative lfq_status; *slot_out_or_null gets the slot (or -1). */
int lfq_device_count(void);
/* Pinned host memory for a producer's track buffers (hipHostMalloc): with it the uploads of lfq_call_snvs_submit(...,
 * tracks_on_device = 0) are DMA transfers at the link's rate that return at once -- pageable memory is staged.  NULL when
 * there is no device / no memory. */
void *lfq_host_alloc(size_t bytes);
void lfq_host_free(void *p);
int lfq_pick_device(int n_devices, int *slot_out_or_null);
void lfq_destroy(lfq_ctx *ctx);
int lfq_synchronize(lfq_ctx *ctx);

/* --- layer 1: kernels --- */
/* All pointers in `tracks` and the outputs are DEVICE pointers.  `d_counts` holds ncols entries;
 * `d_pvals` holds pvals_capacity entries.  `bonf_base` is conf->bonf_subst before this batch.
 * `stream` is a hipStream_t (NULL = the context's own stream).  Asynchronous; `stats` is filled
 * by lfq_batch_finish(), which waits for the batch.
 * ONE batch in flight per context: a batch ends on an internal stream (its DP kernels), and what the library itself
 * queues for the context afterwards (the next batch, a pileup or generator call that rewrites context-owned tracks) is
 * ordered behind the batch's last event -- but the caller's own writes to d_counts / d_pvals / the tracks are not:
 * call lfq_batch_finish() (or pass your stream, into which the batch is then joined) before touching them. */
int lfq_snv_batch_device(lfq_ctx *ctx, const lfq_conf *conf, const lfq_tracks *tracks,
                         lfq_col_counts *d_counts, lfq_col_pvals *d_pvals, int64_t pvals_capacity,
                         void *stream);
int lfq_batch_finish(lfq_ctx *ctx, lfq_batch_stats *stats);

/* --- layer 2: the call_snvs loop --- */
/* tracks_on_device != 0: `tracks` holds device pointers (data resident in HBM);
 * otherwise host pointers, copied to the device first.  Writes at most records_capacity
 * records (column order) and sets *n_records.  Updates conf->bonf_subst / num_snv_tests exactly
 * like the per-column loop of the reference.  `h_counts_or_null`: optional host copy of the dense
 * per-column counts (ncols entries). */
int lfq_call_snvs_batch(lfq_ctx *ctx, lfq_conf *conf, const lfq_tracks *tracks, int tracks_on_device,
                        lfq_snv_record *records, int64_t records_capacity, int64_t *n_records,
                        lfq_col_counts *h_counts_or_null, lfq_batch_stats *stats);

/* --- indel tests (call_indels, lofreq_call.c:619-726) on the same kernels ------------------------------
 * One "test" = one indel event of one column = snpcaller() on all reads of the column with
 * counts = {event count, 0, 0} (lofreq_call.c:306-426).  The caller packs each test as a
 * pseudo-column in the track format: bq = indel quality, baq = indel alignment quality of the tested
 * event's reads (255 elsewhere or with IDAQ off), mq, sq; nt = 1 ('C') for the tested event's reads, 0 for
 * every other read; ref_base = 'A'.  No base filters apply; the running factor is conf->bonf_indel, +1 per
 * test (lofreq_call.c:693-696).  Returns the significant tests (p * bonf_indel < sig) in test order. */
typedef struct lfq_indel_call {
    int64_t test;              /* pseudo-column index within the batch */
    int64_t bonf;              /* bonf_indel at this test */
    long double pvalue;
    int32_t qual;              /* PROB_TO_PHREDQUAL(pvalue) */
    int32_t count;             /* event count (AF numerator, lofreq_call.c:334) */
} lfq_indel_call;
int lfq_indel_batch_device(lfq_ctx *ctx, const lfq_conf *conf, const lfq_tracks *tracks,
                           lfq_col_counts *d_counts, lfq_col_pvals *d_pvals, int64_t pvals_capacity,
                           void *stream);
int lfq_call_indel_tests_batch(lfq_ctx *ctx, lfq_conf *conf, const lfq_tracks *tracks, int tracks_on_device,
                               lfq_indel_call *calls, int64_t calls_capacity, int64_t *n_calls,
                               lfq_batch_stats *stats);
/* --- call_indels drop-in (lofreq_call.c:619-726): the indel fields of a batch of plp_col_t, flattened ----
 * side[0] = insertions, side[1] = deletions.  Events of a column are listed in the order the reference
 * iterates its uthash (insertion order = first occurrence in the pileup, utils.h:101-135).  "Non-event reads"
 * are ins_quals/ins_map_quals (del_quals/del_map_quals): reads of the column carrying no event of that side
 * (plp.c compile_plp_col).  Qualities are phred ints as in the reference; -1 = not available. */
typedef struct lfq_indel_side {
    const int32_t *non_fw, *non_rv;    /* [ncols]     non_ins_fw_rv / non_del_fw_rv (plp.h:127-128) */
    const int64_t *ne_off;             /* [ncols+1]   non-event reads of each column */
    const int16_t *ne_q, *ne_mq;       /*             ins_quals / ins_map_quals (plp.h:113-116) */
    const int64_t *ev_off;             /* [ncols+1]   events of each column */
    const int64_t *key_off;            /* [nevents+1] event key (inserted / deleted sequence) in key_chars */
    const char *key_chars;
    const int32_t *ev_fw, *ev_rv;      /* [nevents]   ins_event.fw_rv (utils.h:108) */
    const int64_t *rd_off;             /* [nevents+1] reads of each event; count = rd_off[e+1]-rd_off[e] */
    const int16_t *rd_q, *rd_aq, *rd_mq, *rd_sq;   /* ins_quals / ins_aln_quals / ins_map_quals / ins_source_quals */
} lfq_indel_side;

typedef struct lfq_indel_columns {
    int64_t ncols;
    const uint8_t *ref_base;
    const int32_t *coverage_plp, *num_tails, *num_non_indels, *num_ins, *num_dels, *hrun;
    lfq_indel_side side[2];
    /* optional (NULL when unknown; not read by lfq_call_indels_batch): 1 where the column's consensus is an
     * insertion or deletion, cons_base[0] == '+' / '-' (plp.c:1236-1270) -- call_vars does not call SNVs there
     * (lofreq_call.c:928-931), see lfq_pileup_skip_snv_columns */
    const uint8_t *cons_indel;
} lfq_indel_columns;

typedef struct lfq_indel_record {
    int64_t col;
    int32_t side;                      /* 0 insertion, 1 deletion */
    int32_t event;                     /* index into side[side]'s event arrays */
    int32_t qual, dp, sb;              /* report_var (lofreq_call.c:95-155) */
    int32_t ref_fw, ref_rv, alt_fw, alt_rv;
    int32_t hrun;
    float af;
    int32_t count;
    int64_t bonf;
    long double pvalue;
} lfq_indel_record;

/* call_indels over a batch of columns, in column/side/event order: gates (min_cov on non_indels+ins+dels,
 * 'N' reference, the poly-AT 1-bp A/T rule of :649-681), packs every surviving event as a pseudo-column,
 * runs them through lfq_call_indel_tests_batch and assembles the report_var fields.  conf->bonf_indel and
 * conf->num_indel_tests are advanced exactly as the reference does. */
int lfq_call_indels_batch(lfq_ctx *ctx, lfq_conf *conf, const lfq_indel_columns *cols,
                          lfq_indel_record *records, int64_t records_capacity, int64_t *n_records,
                          int64_t *n_tests);

/* `lofreq filter` as `lofreq call` invokes it, for indel records (lofreq_filter.c:325-335, 210-236, 599-601):
 * QUAL >= indelqual_thresh (= lfq_snvqual_thresh(sig, bonf_indel), lofreq_call.c:1529-1534; 0 = off), and with
 * the defaults on, DP >= 10.  The strand-bias filter skips indels by default. keep[i] = 1 for PASS. */
int lfq_filter_indel_records(const lfq_indel_record *records, int64_t n, int indelqual_thresh, int apply_defaults,
                             int32_t *keep);

/* vcf_write_var + vcf_var_sprintf_info for an indel record (vcf.c:469-497, 608-629);
 * af = count / ((float)coverage_plp - num_tails), dp = coverage_plp - num_tails (lofreq_call.c:132, 334) */
int lfq_format_indel_record(char *buf, int buflen, const char *chrom, int64_t pos0, const char *ref,
                            const char *alt, int qual, int dp, float af, int sb, int ref_fw, int ref_rv,
                            int alt_fw, int alt_rv, int hrun, const char *filter_or_null);

/* --- base alignment quality: the per-read pre-step -----------------------------------
 * bam_prob_realn_core_ext (bam_md_ext.c:260-491) with baq_flag = 1 for reads without a pre-existing `lb` tag:
 * alignment window and band from the CIGAR, kpa_ext_glocal (kprobaln_ext.c:80-270, kpa_ext_par_lofreq_illumina),
 * then the plain or extended BAQ of every base.  One call = a batch of reads of ONE contig.  The caller
 *  skips unmapped / zero-length reads like the reference (:287-289) and appends
 * lb_out[seq_off[r] .. seq_off[r+1]) as the read's `lb:Z` tag (bytes are BAQ + 33, capped at '~').
 * lfq_baq_idaq_batch additionally computes the indel alignment qualities (idaq, :73-248): ai_out / ad_out get the
 * bytes of the `ai` / `ad` tags ('~' where there is nothing), tag_flags[r] bit 0 / bit 1 say whether read r gets an
 * ai / ad tag at all (n_ins / n_del > 0, :238-243).  More than 64 indels or 1024 repeat cells per read are not tracked.
 * BASE CODES (every `seq` array of this header): 0..3 = A, C, G, T, 4 = N -- seq_nt16_int of the BAM base -- and 5..15 = the
 * other letters of htslib's seq_nt16_str in its order, "=MRSVWYHKDB" (LFQ_SEQ_LETTERS "ACGTN=MRSVWYHKDB"[code]).  A code
 * above 3 behaves like N in the HMM, the pileups and the tests, as it does in the reference; where the reference compares or
 * prints the LETTER of a read base -- the repeat scan of idaq (:197), count_cigar_ops (samutils.c:486-489), the key of an
 * insertion (plp.c:1092-1093) -- an ambiguity code is its own letter.  A caller that only knows "not A, C, G, T" passes 4. */
typedef struct lfq_baq_reads {
    int64_t n_reads;
    const int32_t *pos;        /* [n]   bam1_core_t.pos (0-based leftmost reference coordinate) */
    const int64_t *cigar_off;  /* [n+1] into cigar */
    const uint32_t *cigar;     /*       BAM encoding: len << 4 | op (M0 I1 D2 N3 S4 H5 P6 =7 X8) */
    const int64_t *seq_off;    /* [n+1] into seq / qual / lb_out */
    const uint8_t *seq;        /*       0..3 = A,C,G,T, 4 = anything else (seq_nt16_int of the BAM base) */
    const uint8_t *qual;       /*       phred base qualities */
    const char *ref;           /*       the contig's sequence (faidx_fetch_seq), ASCII */
    int64_t ref_len;
} lfq_baq_reads;
int lfq_baq_batch(lfq_ctx *ctx, const lfq_baq_reads *reads, int baq_extended, uint8_t *lb_out);
int lfq_baq_idaq_batch(lfq_ctx *ctx, const lfq_baq_reads *reads, int baq_extended, uint8_t *lb_out,
                       uint8_t *ai_out, uint8_t *ad_out, uint8_t *tag_flags);

/* --- `lofreq viterbi`: the realignment of the reads with an indel, before alnqual ----------------
 * fetch_func (lofreq_viterbi.c:107-345) + viterbi + left_align_indels (viterbi.c:99-330, 48-96) for a batch of reads of ONE
 * contig, in the read layout of the BAQ call.  The caller skips unmapped reads (:148-151).  Per read, in this order:
 *   1. Left as it is, with the status that says why: an H operation or an operation other than M = X I D S anywhere in the
 *      CIGAR (:188-192, 208-212: the whole read, whatever came before) -> LFQ_VIT_SKIPPED_OP; no I / D operation (:216) ->
 *      LFQ_VIT_NO_INDEL; every query base has quality 2 (:221; also a read without query bases) -> LFQ_VIT_ALL_Q2.  The hidden
 *      --reclip option is not implemented.
 *   2. Query = bases and qualities of the M = X I operations (soft clips dropped, :178-213), compared AS LETTERS
 *      (LFQ_SEQ_LETTERS[code], htslib's seq_nt16_str) with the upper-cased reference (:161): an N in the read equals an N in
 *      the reference.
 *   3. q2def = def_qual (-q), or when that is negative int_median of the query's qualities other than 2 (utils.c:436-457: an
 *      even count gives (a + b) / 2.0 truncated); it stands in for every quality of 2 (viterbi.c:188-192).
 *   4. Window [max(0, pos - 10), min(ref_len, x + 10)), x = pos + the reference bases the CIGAR consumes (:250-259).  The
 *      reference's stack buffer for it (:251) is not a limit here.
 *   5. viterbi(): L = window length + 1 PER READ in the nine transition constants; bp = pow(10, -0.1 q), ep_match =
 *      log10(1 - bp), ep_match_not = log10(bp / 3.), ep_ins = log10(.25); borders (double)INT_MIN, not -inf; argmax_d takes the
 *      FIRST maximum (utils.c:87-98) of the terms in their written order (S M I D / S M I / M D); termination over M then I of
 *      the last query row with `>`; the trace-back stops at a pointer S or at i == 0 || k == 0 and returns that k.  The tables
 *      are computed on the host with the host's libm; the device adds and compares only, so the result is the reference's bit
 *      for bit.
 *   6. left_align_indels on the traced columns, then the run-length CIGAR of M / I / D with the original leading / trailing S
 *      operation put back (:270-304); = and X come back as M.
 *   7. pos = max(0, pos - 10) + k (:316-321).
 * Qualities above 93 in a read that is realigned, def_qual above 93 and a realigned read with pos < 0 are LFQ_ERR_INVALID.
 * What the caller still does: delete the NM / MC / MD / AS tags of EVERY read unless -k (:119-146), write
 * pos and CIGAR back, and sort -- the output is no longer coordinate-sorted (:362).
 * The result belongs to the context and is valid until its next lfq_viterbi_batch or lfq_readset_viterbi call.  cigar[cigar_off[r] .. cigar_off[r + 1])
 * is read r's CIGAR in BAM encoding -- the input's for a read left as it is, so that the arrays can be taken whole. */
#define LFQ_VIT_NO_INDEL 0
#define LFQ_VIT_SKIPPED_OP 1
#define LFQ_VIT_ALL_Q2 2
#define LFQ_VIT_REALIGNED 3
#define LFQ_VIT_STATUS_MASK 7
#define LFQ_VIT_CHANGED 8          /* bit: position or CIGAR differ from the input (only ever set with LFQ_VIT_REALIGNED) */
typedef struct lfq_viterbi_result {
    int64_t n_reads;
    const int32_t *pos;            /* [n] */
    const uint8_t *status;         /* [n] LFQ_VIT_* */
    const int64_t *cigar_off;      /* [n+1] */
    const uint32_t *cigar;
} lfq_viterbi_result;
int lfq_viterbi_batch(lfq_ctx *ctx, const lfq_baq_reads *reads, int def_qual, const lfq_viterbi_result **out);
/* the realignment kernels of the context's last lfq_viterbi_batch call on the device's clock (first launch -> last done),
 * their number (the batch is cut by the scratch budget of the BAQ step), the call's reads and how many were realigned */
typedef struct lfq_viterbi_times {
    float ms_kernels;
    int32_t n_launches;
    int64_t n_reads, n_realigned;
} lfq_viterbi_times;
int lfq_last_viterbi_times(lfq_ctx *ctx, lfq_viterbi_times *t);

/* --- `lofreq indelqual`: the BI / BD per-base indel qualities, between alnqual and call -------------
 * What `--call-indels` reads for every pileup entry (plp.c:1062) and a BAM that has not been through GATK BQSR lacks.  A batch
 * of reads of ONE contig in the read layout of the BAQ call; reads->seq / reads->qual are not read and may be NULL.  bi_out /
 * bd_out get the tag bytes (quality + 33) in the seq_off layout: what lfq_pileup_indel_tags.bi / .bd take.
 *   LFQ_IDQ_UNIFORM (-u INT[,INT]; add_uniform / uniform_fetch_func, lofreq_indelqual.c:69-104, 218-258): every base of every
 *      read gets ENCODE_Q(ins_qual + 33) in BI and ENCODE_Q(del_qual + 33) in BD -- a byte below '!' becomes '!', one above '~'
 *      becomes '~' (:66).  Positions and CIGARs are not looked at, as in the reference.
 *   LFQ_IDQ_DINDEL (--dindel -f ref.fa; dindel_fetch_func, :136-215): the contig is upper-cased (:155) and find_homopolymers
 *      (:109-133) gives every position a count: the run length at the FIRST base of a homopolymer run, 1 everywhere else (runs
 *      of N count).  The CIGAR walk (:173-198) gives a base aligned to reference position x by an M / = / X operation '!' if
 *      x > ref_len - 2, else with c = the count of position x + 1, '!' if c > 18, else "!MMMLKEC@=<;:988776"[c] (DINDELQ, :42);
 *      D advances x; every base of an I or S operation gets '!'; H does nothing.  BI and BD get the same string (:205, 211);
 *      ins_qual / del_qual are not used.  The caller leaves out the reads the reference writes unchanged (UNMAP | SECONDARY |
 *      QCFAIL | DUP, :144).  LFQ_ERR_INVALID for what the reference cannot do: any other operation (N, P, ...: fatal, :195), a
 *      CIGAR whose query length differs from the read's seq_off span (the reference overruns its stack array, :168), pos < 0.
 * An unknown mode is LFQ_ERR_INVALID; an empty batch launches nothing.
 * What the caller still does: the flag mask, deleting old BI / BD tags and appending the new ones as Z tags
 * (l_qseq bytes + NUL), and "Do not realign your BAM file afterwards!" (:332) -- viterbi comes BEFORE this step. */
#define LFQ_IDQ_UNIFORM 1
#define LFQ_IDQ_DINDEL 2
typedef struct lfq_indelqual_conf {
    int32_t mode;                  /* LFQ_IDQ_UNIFORM or LFQ_IDQ_DINDEL */
    int32_t ins_qual, del_qual;    /* uniform mode: the two values of -u (one value given: both the same) */
} lfq_indelqual_conf;
int lfq_indelqual_batch(lfq_ctx *ctx, const lfq_baq_reads *reads, const lfq_indelqual_conf *conf, uint8_t *bi_out,
                        uint8_t *bd_out);
/* the kernels of the context's last lfq_indelqual_batch / lfq_readset_indelqual call on the device's clock, their number, the
 * call's reads and bases */
typedef struct lfq_indelqual_times {
    float ms_kernels;
    int32_t n_launches;
    int64_t n_reads, n_bases;
} lfq_indelqual_times;
int lfq_last_indelqual_times(lfq_ctx *ctx, lfq_indelqual_times *t);

/* --- device-side pileup: reads -> the packed SNV tracks of a region -------------------------
 * What compile_plp_col (plp.c:797-1017) builds per column, for all columns of [region_begin, region_end) at once,
 * directly in HBM in the lfq_tracks layout.  The host has done what mplp_func does per read (plp.c:600-700): flag /
 * MAPQ filtering, and BAQ (lfq_baq_batch) if wanted.  Columns = the covered positions in order (mpileup yields no
 * column for a position without alignments); col_pos_out[c] is the reference position of column c.
 * The returned tracks point into memory owned by the context, valid until the next lfq_pileup_snv_tracks call;
 * they can be handed straight to lfq_call_snvs_batch(..., tracks_on_device = 1, ...). */
typedef struct lfq_pileup_reads {
    int64_t n_reads;
    const int32_t *pos;        /* [n]   bam1_core_t.pos */
    const int64_t *cigar_off;  /* [n+1] */
    const uint32_t *cigar;     /*       BAM encoding */
    const int64_t *seq_off;    /* [n+1] into seq / qual / baq */
    const uint8_t *seq;        /*       0..4 */
    const uint8_t *qual;       /*       phred */
    const uint8_t *baq;        /*       lb tag bytes (BAQ + 33), or NULL (every BAQ missing) */
    const uint8_t *mapq;       /* [n]   bam1_core_t.qual */
    const uint8_t *reverse;    /* [n]   bam_is_rev */
    const char *ref;           /*       the contig */
    int64_t ref_len;
    const uint8_t *sq;         /* [n]   source quality byte of the read (lfq_source_qual_batch), or NULL: no sq track */
} lfq_pileup_reads;
int lfq_pileup_snv_tracks(lfq_ctx *ctx, const lfq_pileup_reads *reads, int64_t region_begin, int64_t region_end,
                          int min_plp_bq, lfq_tracks *tracks_out, int64_t *col_pos_out);

/* The indel fields of compile_plp_col (plp.c:1019-1192) for the same reads: per column (= covered position, the
 * same column numbering as lfq_pileup_snv_tracks) coverage_plp, num_tails, num_non_indels / num_ins / num_dels,
 * hrun (get_hrun, plp.c:744-787), per side the strand counts and -- at columns with at least one event, the only
 * ones call_indels reads them for -- the ins_quals / del_quals arrays of the reads without such an event, and
 * the event tables (key, strands, per-read qualities) in the reference's order (first appearance; reads in pileup
 * order).  Pileup entries follow htslib's resolve_cigar2: an entry inside a deletion / reference skip takes the
 * qualities at the query position of the next base; the indel of an entry is the I / D operation following the
 * last position of its CIGAR operation.  Entries with BI or BD below min_plp_idq are ignored (plp.c:1062).
 * *cols_out points into memory owned by the context, valid until the next lfq_pileup_indel_columns call; it goes
 * straight into lfq_call_indels_batch. */
/* on = 0: lfq_pileup_indel_columns / lfq_readset_pileup_indels keep the ins_quals / del_quals arrays (ne_q, ne_mq: the
 * bulk of an lfq_indel_columns) on the device only -- the pointers in the struct are NULL, ne_off stays valid -- and
 * lfq_call_indels_batch, given that struct while it is still the context's current one, builds its pseudo-columns
 * from the resident copy.  Saves the largest transfer of the reads -> VCF chain.  Default: on = 1. */
int lfq_set_indel_arrays_on_host(lfq_ctx *ctx, int on);

typedef struct lfq_pileup_indel_tags {
    const uint8_t *bi, *bd;    /* per base (seq_off layout): BI / BD tag bytes (quality + 33); NULL = tag absent (quality 0) */
    const uint8_t *ai, *ad;    /* per base: ai / ad tag bytes (lfq_baq_idaq_batch); NULL = absent (-1) */
    const uint8_t *tag_flags;  /* [n] bit 0..3: read has BI / BD / ai / ad; NULL = every read has every non-NULL array */
    const int32_t *sq;         /* [n] source quality of the read or NULL (-1) */
} lfq_pileup_indel_tags;
int lfq_pileup_indel_columns(lfq_ctx *ctx, const lfq_pileup_reads *reads, const lfq_pileup_indel_tags *tags_or_null,
                             int64_t region_begin, int64_t region_end, int min_plp_idq,
                             const lfq_indel_columns **cols_out, int64_t *col_pos_out);

/* call_vars' gate for SNVs (lofreq_call.c:928-931): columns with skip[col] != 0 (e.g. lfq_indel_columns.cons_indel)
 * of the tracks last returned by lfq_pileup_snv_tracks are taken out of the SNV path -- their num_bases becomes
 * 0, which is the other half of the same gate (num_bases * 2 < coverage_plp): no test, no Bonferroni step. */
int lfq_pileup_skip_snv_columns(lfq_ctx *ctx, const uint8_t *skip, int64_t ncols);

/* --- resident read set: the device-side chain of the steps above ---------------------------------------------
 * lfq_readset_create uploads the reads of one contig region once (reads->baq / reads->sq and the BI / BD bytes of
 * `tags` go along when given); the steps below then work on the device copy and leave their per-base results in
 * HBM for the next one -- BAQ / IDAQ -> source quality -> both pileups -> calls -- so that only VCF-sized data
 * comes back.  The host arrays handed to lfq_readset_create must outlive the read set (the sparse host-side
 * steps -- geometry from the CIGARs, the indel event tables -- read them in place).  The host-buffer entry points
 * above (lfq_baq_idaq_batch, lfq_source_qual_batch, lfq_pileup_snv_tracks, lfq_pileup_indel_columns) are these
 * functions around a temporary read set.
 * Completion: lfq_readset_create may return while its copies are still in flight (a helper thread feeds them to an
 * upload stream) and lfq_readset_baq returns when its kernels are queued; every later call on the read set waits for
 * what it needs, lfq_readset_destroy for everything.  The caller sees no difference as long as the host arrays stay
 * as they are until the read set is destroyed (they must outlive it anyway).
 * Pinned arrays (lfq_host_alloc, hipHostMalloc, hipHostRegister): when the per-base arrays -- seq, qual, BI, BD -- are
 * pinned, lfq_readset_create queues every copy as a DMA transfer itself and returns, and what waits for the data is the
 * stream of the kernels that read it, never the calling thread.  Same results either way.
 * A read set belongs to its context: destroy it before lfq_destroy(ctx) (its device allocations go back to the context,
 * which hands them to the next read set -- keep one context per worker from region to region). */
typedef struct lfq_readset lfq_readset;
int lfq_readset_create(lfq_ctx *ctx, const lfq_pileup_reads *reads, const lfq_pileup_indel_tags *tags_or_null,
                       lfq_readset **out);
void lfq_readset_destroy(lfq_readset *rs);
/* lb (and, with want_idaq, ai / ad) of every read, kept on the device; needs reads->qual */
int lfq_readset_baq(lfq_ctx *ctx, lfq_readset *rs, int baq_extended, int want_idaq);
/* source quality; the per-read byte for the sq track stays on the device, sq_out_or_null gets source_qual()'s value */
int lfq_readset_source_qual(lfq_ctx *ctx, lfq_readset *rs, int def_nm_q, int min_bq, const uint8_t *ign_or_null,
                            int32_t *sq_out_or_null);
/* Returns when the scatter pass is QUEUED: ncols, col_pos_out and max_col_obs are final, the tracks themselves are
 * complete in stream order -- lfq_call_snvs_batch(..., tracks_on_device = 1), lfq_pileup_skip_snv_columns and the uniq
 * calls are queued behind them; call lfq_synchronize(ctx) before reading the device memory yourself.  A region worker
 * calls it between the indel pileup and the indel tests: the scatter pass then runs under the host part of the tests. */
int lfq_readset_pileup_snv(lfq_ctx *ctx, lfq_readset *rs, int64_t region_begin, int64_t region_end, int min_plp_bq,
                           lfq_tracks *tracks_out, int64_t *col_pos_out);
int lfq_readset_pileup_indels(lfq_ctx *ctx, lfq_readset *rs, int64_t region_begin, int64_t region_end, int min_plp_idq,
                              const lfq_indel_columns **cols_out, int64_t *col_pos_out);
/* The reads the pileups of this read set take under the context's current lfq_set_max_depth: keep_out_or_null[r] = 1 for a
 * kept read, 0 for a dropped one; *n_kept_out_or_null = how many are kept (every read without a cap).  Decided once per read
 * set and cap value, on the host, and shared by both pileups.  LFQ_ERR_INVALID for unsorted reads under a cap.  A read set
 * created under targets (lfq_set_bed) reports targets and cap together: the reads the BED keeps, and of those the ones the
 * cap keeps (BED first); with targets alone unsorted reads are fine. */
int lfq_readset_kept_reads(lfq_ctx *ctx, lfq_readset *rs, uint8_t *keep_out_or_null, int64_t *n_kept_out_or_null);
/* copies of the resident tags for writing them back to the BAM; NULL = not wanted.  tag_flags as lfq_baq_idaq_batch */
int lfq_readset_fetch_tags(lfq_ctx *ctx, lfq_readset *rs, uint8_t *lb_out, uint8_t *ai_out, uint8_t *ad_out,
                           uint8_t *tag_flags);

/* `lofreq indelqual` as a step of the read set: BI / BD of every read computed on the device copy and kept there, for a read
 * set created WITHOUT them (arrays the caller did upload are superseded: "Both will overwrite any existing values",
 * lofreq_indelqual.c:331).  Every read then counts as having both tags, and lfq_readset_pileup_indels reads them from the
 * device; the one base per indel event its host side needs is evaluated from the contig and the CIGAR, so that no per-base
 * array crosses the link in either direction.  In Dindel mode BI and BD are one array on the device.  Any time after
 * lfq_readset_create and before lfq_readset_pileup_indels; beside a BAQ step that is still running it takes another stream.
 * lfq_indelqual_batch is this step and the fetch below around a temporary read set. */
int lfq_readset_indelqual(lfq_ctx *ctx, lfq_readset *rs, const lfq_indelqual_conf *conf);
/* copies of the resident BI / BD bytes for writing them to the BAM; NULL = not wanted.  LFQ_ERR_INVALID before the step ran */
int lfq_readset_fetch_indelquals(lfq_ctx *ctx, lfq_readset *rs, uint8_t *bi_out, uint8_t *bd_out);

/* `lofreq viterbi` as a step of the read set, BEFORE every other step: the reads of `rs` are realigned, read by read exactly as
 * lfq_viterbi_batch documents above (classification, query, q2def, window, Viterbi, left-alignment, new CIGAR, new pos, the same
 * LFQ_ERR_INVALID cases), and *out is a NEW read set of the same reads with the new positions and CIGARs, STABLY SORTED BY NEW
 * POSITION (ties keep their input order) -- ready for lfq_readset_baq / _indelqual / the pileups.  The input need not be sorted.
 *   *result_or_null   the struct lfq_viterbi_batch gives for these reads, in the INPUT order; the context's, valid until its
 *                     next viterbi call of either kind.
 *   *order_or_null    [n] order[j] = input index of the read at place j of *out; owned by *out, valid until it is destroyed.
 * `rs` is never modified: it stays valid and usable.  *out owns host copies of everything its host-side steps read (positions,
 * CIGARs, offsets, mapq, strand, bases, qualities, uploaded BI / BD, the contig), made on the host from the caller's arrays in the
 * new order; it depends neither on `rs` nor on the caller's arrays after the call, which need only outlive `rs` as before.  Both
 * read sets are destroyed by the caller, in either order, before lfq_destroy.
 * The per-base device arrays of *out (bases, qualities, uploaded BI / BD) are written ON THE DEVICE from those of `rs`: what
 * crosses the link is per-read descriptors, the new positions, offsets and CIGARs going down and the traced states coming back.
 * Uploaded BI / BD are carried along read by read as they are; that they still fit is the caller's business, as in the
 * reference ("Do not realign your BAM file afterwards!", lofreq_indelqual.c:332).
 * LFQ_ERR_INVALID: a read set created with reads->baq, reads->sq, tags->ai / ->ad / ->sq, or on which lfq_readset_baq,
 * _source_qual or _indelqual has run (all of these depend on the alignment); def_qual > 93; out == NULL.
 * n == 0 or no read to realign: no realignment kernel is launched (lfq_last_viterbi_times: n_launches 0) and *out is the input
 * in its stable-sorted order.  The call blocks until *out is complete. */
int lfq_readset_viterbi(lfq_ctx *ctx, lfq_readset *rs, int def_qual, lfq_readset **out,
                        const lfq_viterbi_result **result_or_null, const int64_t **order_or_null);

/* The read set of BAM records AS THEY LIE IN MEMORY: decoding them -- 4-bit bases -> base codes, qualities, the BI / BD strings
 * among the aux fields -- is done on the device, and the record bytes cross the link once instead of four unpacked per-base arrays.
 * *out equals in every observable way the read set lfq_readset_create builds from the arrays a per-base host loop would make:
 *   base code   0..4 = A C G T N, 5..15 = the other letters, from the nibble through the table {5,0,1,6,2,7,8,9,3,10,11,12,13,14,15,4}
 *               ("=ACMGRSVTWYHKDBN"; high nibble first);
 *   qualities   copied as they are, 0xff included;
 *   BI / BD     from the FIRST aux field with that tag, and only if its type is Z, its string has at least l_qseq bytes before the
 *               NUL and the NUL lies inside the record; otherwise the read has no such tag (tag_flags bit 0 / 1 clear, bytes '!').
 *               The read set has a BI (BD) array exactly when at least one read has the tag.  lb / ai / ad / sq tags are not read (lb / ai / ad: lfq_readset_create_from_bam_tags below);
 *   reverse     flag >> 4 & 1; mapq as given.
 * Ownership: *out owns host copies of everything its host-side steps read (positions, offsets, CIGARs, mapq, strand, flags, and the
 * per-base arrays, which come back from the device into pinned memory); after the call it depends neither on recs->data nor on the
 * descriptor arrays.  Only `ref` is borrowed.  Every step of a read set runs on it, lfq_readset_viterbi included.
 * The host reads per read only (descriptor checks, prefix sums, the CIGAR words); `data` goes down in one copy -- from the caller's
 * memory if that is pinned (lfq_host_alloc), through a pinned staging copy otherwise.  The call blocks until *out is complete.
 * LFQ_ERR_INVALID, before a device is touched: a NULL ctx, recs or out; n_reads < 0; a NULL array with n_reads > 0; decreasing
 * data_off; l_qseq < 0; a record shorter than l_qname + 4 n_cigar + (l_qseq + 1) / 2 + l_qseq.  LFQ_ERR_INVALID from the decode
 * (*out = NULL, the context stays usable): an aux field of an unknown type or B subtype (A c C s S i I f Z H B are known), a field
 * that runs past its record, a Z / H field without a NUL inside the record.  No device read leaves [data_off[r], data_off[r + 1])
 * by more than the aligned dword around its first / last byte, inside the library's own buffer.
 * n_reads == 0: LFQ_OK, an empty read set, nothing launched. */
typedef struct lfq_bam_records {
    int64_t n_reads;
    const uint8_t *data;      /* bam1_t.data of every read, concatenated: qname | cigar (uint32 LE) | seq, 4-bit, two bases per byte,
                                 high nibble first | qual | aux.  = the bytes of an on-disk BAM record from read_name on.  No alignment
                                 required, neither of data nor of any record. */
    const int64_t *data_off;  /* [n + 1] */
    const int32_t *pos;       /* [n] core.pos */
    const uint16_t *flag;     /* [n] core.flag; only bit 16 (reverse) is read */
    const uint8_t *mapq;      /* [n] core.qual, already capped by the caller (-M) */
    const uint16_t *l_qname;  /* [n] core.l_qname: NUL and htslib's padding included */
    const uint32_t *n_cigar;  /* [n] */
    const int32_t *l_qseq;    /* [n] */
    const char *ref;          /* the contig, borrowed: must outlive the read set, as for lfq_readset_create */
    int64_t ref_len;
} lfq_bam_records;
int lfq_readset_create_from_bam(lfq_ctx *ctx, const lfq_bam_records *recs, lfq_readset **out);
/* copies of a read set's resident per-base inputs, read back from the device: base codes, qualities, BI / BD bytes ('!' throughout
 * for an array the read set does not have) in the seq_off layout, and per read bit 0 / 1 = has BI / BD.  NULL = not wanted.  Any
 * read set; LFQ_ERR_INVALID for BI / BD / flags after lfq_readset_indelqual (lfq_readset_fetch_indelquals has those). */
int lfq_readset_fetch_bases(lfq_ctx *ctx, lfq_readset *rs, uint8_t *seq_out, uint8_t *qual_out, uint8_t *bi_out, uint8_t *bd_out,
                            uint8_t *tag_flags_out);
/* the context's last lfq_readset_create_from_bam on the device's clock: the copy of the records (and descriptors) down, the two
 * kernels (aux pass + base pass), the per-base arrays back into the read set's pinned host copies */
typedef struct lfq_bam_decode_times {
    double upload_ms, kernels_ms, download_ms;
    int64_t n_reads, n_bases, n_data_bytes;
    int n_launches;
} lfq_bam_decode_times;
int lfq_last_bam_decode_times(lfq_ctx *ctx, lfq_bam_decode_times *t);

/* The decode above that also KEEPS the alignment qualities a record already carries, for lfq_readset_baq_fill below: what
 * `lofreq call` does with a BAM that went through `lofreq alnqual` (bam_prob_realn_core_ext under baq_flag = 1, plp.c:667-683).
 *   read_tags   LFQ_BAM_READ_LB: the first lb field of every record; LFQ_BAM_READ_IDAQ: the first ai and the first ad field.
 *               0: lfq_readset_create_from_bam in every observable way.  An unknown bit: LFQ_ERR_INVALID before a device is touched.
 * For a selected tag the FIRST aux field with that tag decides (bam_aux_get, as for BI / BD): no such field -- the read has no
 * stored tag; a field of type Z with at least l_qseq bytes before its NUL -- its first l_qseq bytes are the read's stored tag (the
 * pileup indexes the string with qpos).  A first field of another type or with a shorter string: LFQ_ERR_INVALID from the decode,
 * *out = NULL, the context stays usable -- the reference counts such a field as present and reads past it (plp.c:865-897), so
 * there is no defined result to reproduce.  A malformed aux block is refused as by the plain decode, and no device read leaves a
 * record by more than that decode allows.
 * The stored strings wait on the device, in side arrays of the read set; until lfq_readset_baq_fill nothing sees them but
 * lfq_readset_fetch_stored_tags: lfq_readset_fetch_tags, the pileups and lfq_readset_baq (which recomputes every read, as always)
 * behave as on any fresh read set.  lfq_readset_viterbi on a read set of which a read has a stored tag is LFQ_ERR_INVALID: the
 * tags depend on the alignment, as its other refusals do. */
#define LFQ_BAM_READ_LB   1   /* keep the first lb field of every record */
#define LFQ_BAM_READ_IDAQ 2   /* keep the first ai and the first ad field */
int lfq_readset_create_from_bam_tags(lfq_ctx *ctx, const lfq_bam_records *recs, unsigned read_tags, lfq_readset **out);
/* the stored tags, from the device: per-base arrays in the seq_off layout ('!' throughout for a read without the tag), and one
 * byte per read: bit 0 / 1 / 2 = lb / ai / ad stored.  NULL = not wanted.  Any read set (one without stored tags: '!' and 0). */
int lfq_readset_fetch_stored_tags(lfq_ctx *ctx, lfq_readset *rs, uint8_t *lb_out, uint8_t *ai_out, uint8_t *ad_out,
                                  uint8_t *stored_flags_out);
/* lfq_readset_baq that runs the HMM only where a tag is missing: bam_prob_realn_core_ext under baq_flag = 1 (redo_baq: 2, `lofreq
 * call -D`) and idaq_flag = want_idaq.  For read r let S_lb, S_ai, S_ad be its stored bits -- S_lb counts as 0 under redo_baq, S_ai
 * and S_ad as 0 without want_idaq or on a read set decoded without LFQ_BAM_READ_IDAQ -- and has_ins / has_del whether its CIGAR has
 * an I / D operation:
 *   need_r = !S_lb || (want_idaq && ((has_del && !S_ad) || (has_ins && !S_ai)))          (bam_md_ext.c:352-366)
 * (without want_idaq the reference may still run the HMM for a read with S_lb; nothing of that run is used).  The HMM runs for
 * the reads with need_r only; it is lfq_readset_baq's: same kernels, same routes, same bytes.  The resident result:
 *   lb        the stored bytes if S_lb, else the computed ones (:409, :472: an existing tag is never replaced);
 *   ai (ad)   with want_idaq: the stored bytes if S_ai (S_ad); otherwise the computed ones if need_r and the kernel wrote the tag
 *             for the read, else absent ('~' bytes, flag clear).  The reference appends a computed duplicate behind a stored ai /
 *             ad (:241-246); the pileup reads the first field, so the stored one wins here too.
 * tag_flags bits 2 / 3 of a read mean "stored or computed".  Afterwards the read set cannot be told, by the pileups,
 * lfq_readset_fetch_tags, source quality or the calls, from one that was given these arrays.  (redo_baq with TWO lb fields in a
 * record: the reference deletes the first and then reads the second; here the read counts as having none.  Records that
 * `lofreq alnqual` wrote have one.)
 * No read needs the HMM: no HMM kernel is launched and lfq_last_baq_times is left as it was.  A read set without stored tags: the
 * call is lfq_readset_baq.  Returns when its work is queued, like lfq_readset_baq.
 * LFQ_ERR_INVALID: a second fill or BAQ pass that newly wants ai / ad (as lfq_readset_baq).  After a fill that merged stored tags,
 * lfq_readset_encode_bam with LFQ_BAM_PUT_LB / LFQ_BAM_PUT_IDAQ is LFQ_ERR_INVALID: `lofreq alnqual` appends COMPUTED duplicates
 * there, which a filled read set no longer holds -- alnqual on the device stays the full recompute (lfq_readset_baq). */
int lfq_readset_baq_fill(lfq_ctx *ctx, lfq_readset *rs, int baq_extended, int want_idaq, int redo_baq);
/* the context's last lfq_readset_baq_fill (waits for its kernels): n_stored_* count the reads whose stored tag was taken (after
 * redo_baq / want_idaq); n_hmm_launches and ms_hmm are lfq_last_baq_times' figures of the call, 0 when no read needed the HMM;
 * ms_merge: the merge pass */
typedef struct lfq_baq_fill_stats {
    int64_t n_reads, n_need_hmm, n_stored_lb, n_stored_ai, n_stored_ad;
    int32_t n_hmm_launches, pad;
    float ms_hmm, ms_merge;
} lfq_baq_fill_stats;
int lfq_last_baq_fill_stats(lfq_ctx *ctx, lfq_baq_fill_stats *s);

/* The way back: the results of a read set's steps WRITTEN INTO THE BYTES OF BAM RECORDS on the device -- what `lofreq viterbi`,
 * `lofreq alnqual` and `lofreq indelqual` do to a record with bam_aux_get / bam_aux_del / bam_aux_append and replace_cigar -- so
 * that one copy of the original records goes down and one blob of rewritten records comes back, instead of three to five per-base
 * arrays and a memmove per deleted or appended field on the calling thread.
 *   recs          the ORIGINAL records, in the struct of the decode (ref / ref_len are not read);
 *   src_or_null   src[j] = the record of read j of `rs`; NULL = the identity.  After lfq_readset_viterbi: its `order`;
 *   what          LFQ_BAM_* bits, at least one.
 * Output record j = qname | cigar | seq | qual | aux', made from record src[j]; qname, seq and qual are copied byte for byte, and
 * l_qname, l_qseq, flag and mapq of the output record are those of record src[j].  aux' = the surviving fields of the record in
 * their order, then the appended ones in the order lb, ai, ad, BI, BD, each as tag 'Z' <l_qseq bytes> NUL.  "The first field" of a
 * tag is the first aux field with that tag in record order WHATEVER ITS TYPE (bam_aux_get); later fields with the same tag are
 * never touched.
 *   LFQ_BAM_PUT_ALIGNMENT   CIGAR words, n_cigar and pos come from the read set, for every read (replace_cigar,
 *                           lofreq_viterbi.c:340); without it they are the record's.
 *   LFQ_BAM_DROP_ALN_TAGS   `lofreq viterbi` without -k: the first NM, MC, MD and AS field of EVERY record is removed, any type,
 *                           unmapped reads included (lofreq_viterbi.c:119-146).
 *   LFQ_BAM_PUT_LB, LFQ_BAM_PUT_IDAQ, LFQ_BAM_KEEP_EXISTING   `lofreq alnqual`, only for records with !(flag & 4) and l_qseq > 0;
 *                           the others pass through (bam_md_ext.c:291).  For t in lb, ai, ad let F_t be the first field of the
 *                           tag.  Without KEEP_EXISTING (= alnqual -r): if t is selected -- lb by PUT_LB, ai and ad by PUT_IDAQ --
 *                           and F_t is of type Z, F_t is removed and P_t = false; otherwise P_t = (F_t exists), so a non-Z lb is
 *                           neither removed nor replaced (:297-314).  With KEEP_EXISTING nothing is removed and P_t = (F_t
 *                           exists).  has_ins / has_del = the read set's CIGAR of the read has an I / D operation.  Nothing is
 *                           appended when (!PUT_LB || P_lb) && (!has_del || P_ad) && (!has_ins || P_ai) (:352-366; the removals
 *                           stand).  Otherwise lb is appended iff PUT_LB && !P_lb (:409, :472), and with PUT_IDAQ && (has_ins ||
 *                           has_del) ai is appended iff the read got an ai tag and ad iff it got an ad tag (tag_flags of
 *                           lfq_readset_fetch_tags; :241-246) -- WHATEVER P_ai / P_ad say: the reference can duplicate a tag
 *                           here, and so does this.
 *   LFQ_BAM_PUT_INDELQUAL   `lofreq indelqual`: the first BI and the first BD field are removed, any type, and BI then BD are
 *                           appended from the read set's computed qualities -- in uniform mode for every record, unmapped and
 *                           empty ones included (lofreq_indelqual.c:69-104), in Dindel mode for records with !(flag & 0x704)
 *                           only, the others pass through (:143-148).
 * With several bits set the result is that of the reference commands run one after the other (their tag sets are disjoint).
 * What is still missing for a file: the core fields in front of each record -- block_size, refID, pos and n_cigar from the
 * result, mate fields -- and core.bin, which depends on the new pos and CIGAR: lfq_bam_frame_encoded below puts them there; and
 * BGZF: lfq_bgzf_deflate.
 * *out is the context's: valid until its next encode or lfq_destroy.  The call blocks until the blob is complete.
 * LFQ_ERR_INVALID, before a device is touched: a NULL ctx, rs, recs or out; what == 0, an unknown bit, KEEP_EXISTING without
 * PUT_LB / PUT_IDAQ; the descriptor cases of the decode (ref aside) and a record of 2^31 bytes or more; a read set of another
 * context; recs->n_reads different from the read set's; src not a permutation of 0 .. n-1; recs->l_qseq[src[j]] different from the
 * length of read j; PUT_LB on a read set without lb (no lfq_readset_baq), PUT_IDAQ without ai / ad (no lfq_readset_baq with
 * want_idaq), PUT_INDELQUAL before lfq_readset_indelqual.  LFQ_ERR_INVALID from the device (*out = NULL, the context stays
 * usable): a malformed aux block, the cases of the decode.  n_reads == 0: LFQ_OK, an empty result, nothing launched. */
#define LFQ_BAM_PUT_ALIGNMENT  1
#define LFQ_BAM_DROP_ALN_TAGS  2
#define LFQ_BAM_PUT_LB         4
#define LFQ_BAM_PUT_IDAQ       8
#define LFQ_BAM_KEEP_EXISTING 16
#define LFQ_BAM_PUT_INDELQUAL 32
typedef struct lfq_bam_encoded {
    int64_t n_reads;
    const uint8_t *data;      /* the records from read_name on, concatenated, in the READ SET's read order (pinned memory) */
    const int64_t *data_off;  /* [n + 1], data_off[0] = 0 */
    const int64_t *src;       /* [n] index in recs of the record read j was made from */
    const int32_t *pos;       /* [n] core.pos to write */
    const uint32_t *n_cigar;  /* [n] core.n_cigar to write */
} lfq_bam_encoded;
int lfq_readset_encode_bam(lfq_ctx *ctx, lfq_readset *rs, const lfq_bam_records *recs, const int64_t *src_or_null,
                           unsigned what, const lfq_bam_encoded **out);
/* the context's last lfq_readset_encode_bam on the device's clock: the records and descriptors down, the two kernels (plan pass +
 * copy pass), the blob back into pinned memory */
typedef struct lfq_bam_encode_times {
    double upload_ms, kernels_ms, download_ms;
    int64_t n_reads, n_in_bytes, n_out_bytes;
    int n_launches;
} lfq_bam_encode_times;
int lfq_last_bam_encode_times(lfq_ctx *ctx, lfq_bam_encode_times *t);

/* --- BGZF blocks inflated on the device: the step in front of lfq_readset_create_from_bam ------------------------------------------
 * A BAM file is a series of BGZF blocks (SAM specification section 4.1), each a gzip member of at most 65536 bytes that inflates
 * to at most 65536.  lfq_bgzf_inflate takes the blocks of a region as they lie in the file: they go down the link compressed, one
 * launch inflates them (raw deflate, RFC 1951: stored, fixed and dynamic blocks; lofreq_amd/csrc/lfq_inflate.h) and checks each
 * block's CRC-32 and ISIZE against its trailer, and the inflated bytes come back -- and stay on the device as well, see below.
 *
 * The host walks the block headers: ID1 ID2 = 31 139, CM = 8, FLG with FEXTRA, and among the extra subfields -- wherever it stands
 * -- the one with SI1 SI2 = 'B' 'C' and SLEN 2, whose value + 1 is the block's size; ISIZE is the block's last four bytes.
 * LFQ_ERR_INVALID, before a device is touched: a NULL ctx or out, n_bytes < 0, a NULL comp with n_bytes > 0; a bad magic, CM or
 * FLG; a subfield that runs past XLEN; no BC subfield; a block shorter than its own header plus trailer; a header or a block
 * that runs past n_bytes; an ISIZE above 65536.
 * The compressed bytes go down in one copy, from the caller's memory if it is pinned and through a pinned staging area otherwise.
 * The empty block (the 28-byte end-of-file marker, ISIZE 0) is an ordinary block; bytes between the end of the final deflate block
 * and the trailer are ignored; n_bytes == 0 is LFQ_OK with an empty result and nothing launched.
 *
 * status[b] is 0 or the first thing found wrong with block b:
 *   1 malformed deflate data (block type 3, a stored block whose LEN is not ~NLEN, an over-subscribed or incomplete code -- a single
 *     code of one bit excepted, as in zlib --, a 16-repeat with nothing to repeat, a repeat past the last length, no end-of-block
 *     code, a code that is not assigned, length symbol 286 / 287, distance symbol 30 / 31)
 *   2 the input ends inside a symbol, a block header or a stored block
 *   3 a symbol would write past ISIZE
 *   4 a match reaches before the first byte of the block's own output (BGZF blocks share no history)
 *   5 the stream ends with fewer than ISIZE bytes written
 *   6 the CRC-32 of the output is not the trailer's
 * Each is decided from the positions before anything is read or written: the kernel terminates on any input, no load leaves a
 * block's compressed bytes by more than the aligned dword around its first / last byte inside the library's own buffer, and no
 * store leaves [data_off[b], data_off[b] + ISIZE_b).  The bytes of a block with a nonzero status are unspecified; the other blocks
 * of the call are intact.  Any nonzero status: LFQ_ERR_INVALID with *out still pointing at the result, so that status[] can be
 * read; the context stays usable.
 *
 * The result is the context's, valid until its next lfq_bgzf_inflate or lfq_destroy.  Until then the inflated bytes also STAY ON
 * THE DEVICE: lfq_readset_create_from_bam(_tags) and lfq_readset_encode_bam on this context, given records whose `data` lies inside
 * result->data, copy them device to device instead of across the link again (n_decodes_from_device counts such calls).  Blocks. */
typedef struct lfq_bgzf_result {
    int64_t n_blocks;
    const int64_t *comp_off;   /* [n_blocks + 1] offsets of the blocks in the input */
    const int64_t *data_off;   /* [n_blocks + 1] offsets of their output in data (prefix sums of ISIZE) */
    const int32_t *status;     /* [n_blocks] 0 = ok */
    const uint8_t *data;       /* the inflated bytes, pinned host memory, the context's */
    int64_t n_bytes;
} lfq_bgzf_result;
int lfq_bgzf_inflate(lfq_ctx *ctx, const uint8_t *comp, int64_t n_bytes, const lfq_bgzf_result **out);
/* the context's last lfq_bgzf_inflate on the device's clock: the compressed bytes and block descriptors down, the kernel, statuses
 * and inflated bytes back into pinned memory; n_decodes_from_device: the decode / encode calls since then that took their records
 * from the resident inflated bytes */
typedef struct lfq_bgzf_times {
    double upload_ms, kernels_ms, download_ms;
    int64_t n_blocks, n_in_bytes, n_out_bytes;
    int n_launches, n_decodes_from_device;
} lfq_bgzf_times;
int lfq_last_bgzf_times(lfq_ctx *ctx, lfq_bgzf_times *t);

/* The records of inflated BAM bytes, located and filtered as sam_itr_next + mplp_func (plp.c:606-722) keep them.  Host only, no
 * context.  bam[first .. stop) is a chain of records as they lie in the file: block_size (int32) and that many bytes, of which the
 * first 32 are the core (refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen).  `first` points
 * behind the file's header (magic, text, references), which stays the caller's, as does MPLP_ILLUMINA13.  BED overlap is not
 * this scan's either: the read set made from the records applies the context's targets (lfq_set_bed), masking reads, not removing
 * records.
 * A record is kept when, in this order:
 *   refID >= 0, and refID == tid when tid >= 0;
 *   !(flag & flag_mask)                                             (unmapped, secondary, QC fail, duplicate: plp.c:613-624);
 *   pos < end && endpos > beg, endpos = pos + the reference bases of the CIGAR (M D N = X), or pos + 1 when that is 0 (bam_endpos);
 *   mapq > max_mq: the mapq handed out is max_mq; otherwise mapq < min_mq drops the record; otherwise, with no_orphan, a paired
 *     read (flag 1) without the proper-pair bit (flag 2) is dropped -- the reference's else-if chain (plp.c:707-721);
 *   l_seq > 0 and n_cigar_op > 0                                    (as lfq_region_add_record drops the others).
 * (*out)->recs describes the kept records where they lie: data = bam, data_off[r] = the record's read_name, data_off[n_reads] =
 * the end of the last kept record (`first` when none is kept).  Records in a file do not abut -- the next one's block_size and
 * core, and the dropped records, lie between -- so record r is [data_off[r], data_end[r]) and NOT [data_off[r], data_off[r + 1]):
 * lfq_readset_create_from_bam_scan and lfq_readset_create_from_bgzf decode with data_end; lfq_readset_create_from_bam takes
 * records that abut.
 * n_seen: the complete records walked; n_consumed: the offset of the first record that does not end before `stop` (a chunk may end
 * inside a record or its block_size: the caller carries the tail over; LFQ_OK).
 * LFQ_ERR_INVALID (*out = NULL): a NULL bam, o or out; first < 0, stop < first; block_size < 32; l_seq < 0 or a record whose
 * l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq exceeds its block_size - 32. */
typedef struct lfq_bam_scan_opts {
    int32_t tid;               /* -1 = any */
    int64_t beg, end;          /* 0-based, half-open */
    int min_mq, max_mq, no_orphan;
    unsigned flag_mask;
} lfq_bam_scan_opts;
/* tid -1, beg 0, end INT64_MAX, min_mq 0, max_mq 255, no_orphan 0, flag_mask 4 | 256 | 512 | 1024 */
void lfq_bam_scan_opts_init(lfq_bam_scan_opts *o);
typedef struct lfq_bam_scan {
    lfq_bam_records recs;      /* the kept records; ref / ref_len are 0 for the caller to set */
    const int64_t *data_end;   /* [n_reads] one past the last byte of record r */
    int64_t n_seen, n_consumed;
} lfq_bam_scan;
int lfq_bam_scan_records(const uint8_t *bam, int64_t first, int64_t stop, const lfq_bam_scan_opts *o, lfq_bam_scan **out);
void lfq_bam_scan_free(lfq_bam_scan *s);
/* lfq_readset_create_from_bam_tags on the records of a scan -- or of any lfq_bam_scan the caller fills in, such as the kept
 * records of several scans over one buffer (integration/lofreq_amd_region.c) --: record r is [data_off[r], data_end[r]), with
 * data_end[r] <= data_off[r + 1]; recs.ref / ref_len set by the caller; n_seen and n_consumed are not read.  Records inside the
 * context's live lfq_bgzf_inflate result are taken from the device copy.  Everything else as lfq_readset_create_from_bam_tags. */
int lfq_readset_create_from_bam_scan(lfq_ctx *ctx, const lfq_bam_scan *scan, unsigned read_tags, lfq_readset **out);

/* lfq_bgzf_inflate + lfq_bam_scan_records over [first, stop_or_neg) of the inflated bytes (negative: to their end) +
 * lfq_readset_create_from_bam_tags on the kept records, whose bytes are taken from the device copy of the inflated data: in every
 * observable way that decode on those records.  *n_consumed_or_null: the scan's n_consumed.  Errors of the three steps as they
 * return them; *out = NULL then. */
int lfq_readset_create_from_bgzf(lfq_ctx *ctx, const uint8_t *comp, int64_t n_bytes, int64_t first, int64_t stop_or_neg,
                                 const lfq_bam_scan_opts *o, const char *ref, int64_t ref_len, unsigned read_tags,
                                 lfq_readset **out, int64_t *n_consumed_or_null);

/* --- the last two steps of writing a BAM: the records framed, the bytes cut into BGZF blocks and compressed -----------------------
 * lfq_bam_frame_encoded makes the BODY OF A BAM FILE from the context's last lfq_readset_encode_bam result, which is still on the
 * device.  cores: 32 bytes per ORIGINAL record, as they lie in the file behind block_size (refID, pos, l_read_name, mapq, bin,
 * n_cigar_op, flag, l_seq, next_refID, next_pos, tlen), indexed through the result's `src`.  Record j of the output is
 *     block_size (int32 = 32 + the record's length) | core' | the record's bytes
 * where core' is cores[src[j]] with three fields replaced: pos and n_cigar_op from the encode result, and bin; everything else --
 * refID, mapq, flag, l_read_name, l_seq, the mate fields -- is copied.  bin is the SAM specification's reg2bin of [pos, end)
 * (section 5.3), end = pos + the reference bases (M D N = X) of the CIGAR words in the output record; the alignment counts as
 * length 1 when that is 0 or the read is unmapped (flag 4), as section 4.2 says, so pos = -1 gives 4680.  The reference never
 * sets core.bin after replace_cigar: the bin here is the specification's, not necessarily the 2.1.4 binary's.
 * Two launches: one lane per read computes end and bin, a gather pass writes the body.  The body comes back into pinned memory AND
 * STAYS ON THE DEVICE, so that lfq_bgzf_deflate given framed->data (or a part of it) takes it from there.
 * LFQ_ERR_INVALID: a NULL argument; no live encode result on the context; n_cores <= an index in src; a core whose l_read_name or
 * l_seq is not that of the record it is put in front of; a record with more than 65535 CIGAR operations.  n_reads == 0: LFQ_OK,
 * an empty result, nothing launched.  *out is the context's: valid until its next frame or encode, or lfq_destroy.  Blocks. */
typedef struct lfq_bam_framed {
    int64_t n_reads;
    const int64_t *rec_off;    /* [n + 1] where record j (its block_size) starts in data */
    const uint8_t *data;       /* the body, pinned host memory, the context's */
    int64_t n_bytes;
} lfq_bam_framed;
int lfq_bam_frame_encoded(lfq_ctx *ctx, const uint8_t *cores, int64_t n_cores, const lfq_bam_framed **out);

/* lfq_bgzf_deflate cuts `data` into BGZF blocks (SAM specification section 4.1) and compresses every block on the device: raw
 * deflate (RFC 1951; lofreq_amd/csrc/lfq_deflate.h), one stream of one final block per BGZF block -- the smallest, by exact bit
 * count, of a stored block (5 + n bytes), one with the fixed codes and one with dynamic codes over an LZ77 match search (lengths 3
 * to 258, distances up to 32768) inside the block; ties go to the lower type.  There are no compression levels.
 *   cuts_or_null  NULL: a block every 65280 bytes (htslib's BGZF_BLOCK_SIZE: a stored block of it still fits BSIZE).  Otherwise
 *                 n_cuts strictly increasing offsets inside (0, n_bytes): the blocks are the pieces between them, each at most
 *                 65280 bytes -- for a caller that wants no record split across blocks, or virtual offsets for an index: byte
 *                 p of data lies in the block b with data_off[b] <= p < data_off[b + 1], and its virtual offset is
 *                 (file offset of comp + comp_off[b]) << 16 | (p - data_off[b]);
 *   flags         LFQ_BGZF_PUT_EOF appends the 28-byte end-of-file marker.
 * Every block is the 18 header bytes 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 and BSIZE - 1, as htslib writes them, the
 * stream, and CRC-32 and ISIZE of its payload, both computed on the device.  The bytes written depend on the payload alone: the
 * host program lofreq_amd/csrc/lfq_deflate_check.cpp prints the same streams.
 * The input goes down in one copy, from the caller's memory if it is pinned and through a pinned staging area otherwise -- unless
 * `data` lies inside the context's live lfq_bgzf_inflate result or inside its live lfq_bam_frame_encoded result: then the payload is
 * taken from the device copy (n_from_device = 1).  Two launches: one wavefront per block compresses into a slot of the block's
 * own; eight bytes a block come back, from which comp_off follows; a second kernel writes header, stream and trailer to their
 * final places; one copy brings comp back.  The kernel terminates on every input, loads nothing outside the aligned dwords around
 * a block's payload inside the library's own buffers and stores nothing outside the block's slot.
 * LFQ_ERR_INVALID, before a device is touched: a NULL ctx or out; n_bytes < 0; NULL data with n_bytes > 0; an unknown flag bit;
 * NULL cuts with n_cuts > 0; n_cuts < 0; cuts not strictly increasing inside (0, n_bytes); a piece above 65280 bytes.
 * n_bytes == 0: LFQ_OK, no blocks, nothing launched; comp is then just the marker when LFQ_BGZF_PUT_EOF is set.
 * *out is the context's: valid until its next lfq_bgzf_deflate or lfq_destroy.  Blocks. */
#define LFQ_BGZF_PUT_EOF 1
typedef struct lfq_bgzf_deflated {
    int64_t n_blocks;          /* the end-of-file marker not counted */
    const int64_t *data_off;   /* [n_blocks + 1] block b holds input bytes [data_off[b], data_off[b + 1]) */
    const int64_t *comp_off;   /* [n_blocks + 1] where block b starts in comp */
    const uint8_t *btype;      /* [n_blocks] 0 stored, 1 fixed, 2 dynamic */
    const uint8_t *comp;       /* the blocks, then the marker if asked for; pinned host memory, the context's */
    int64_t n_bytes;           /* all of comp */
} lfq_bgzf_deflated;
int lfq_bgzf_deflate(lfq_ctx *ctx, const uint8_t *data, int64_t n_bytes, const int64_t *cuts_or_null, int64_t n_cuts,
                     unsigned flags, const lfq_bgzf_deflated **out);
/* the context's last lfq_bgzf_deflate on the device's clock: the input and the offsets down, the two kernels, sizes and blocks back
 * into pinned memory; n_from_device: 1 when the input was taken from a resident result */
typedef struct lfq_bgzf_deflate_times {
    double upload_ms, kernels_ms, download_ms;
    int64_t n_blocks, n_in_bytes, n_out_bytes;
    int n_launches, n_from_device;
} lfq_bgzf_deflate_times;
int lfq_last_bgzf_deflate_times(lfq_ctx *ctx, lfq_bgzf_deflate_times *t);

/* --- the index of a BAM: its .bai built on the device, written, read and queried ---------------------------------------------------
 * lfq_bam_index_build makes the index of the records body[rec_off[j] .. rec_off[j + 1]), j < n_recs, that lie in BGZF blocks whose
 * tables are data_off / comp_off ([n_blocks + 1] each, as lfq_bgzf_deflated and lfq_bgzf_result give them): block b holds bytes
 * [data_off[b], data_off[b + 1]) of body and starts at byte comp_off[b] + file_off of the file -- file_off lets the caller put the
 * header's blocks in front.  rec_off and data_off count bytes of body; the records need not start at data_off[0] (a header inside
 * the first blocks).  n_ref: the references of the file's header.
 * The index is the one `lofreq index` of the reference's 2.1.4 binary writes, bin for bin and chunk for chunk: INTEGRATION.md
 * section 13 states the seven rules and tests/golden/bai_binary.json holds them to the binary.  Work proportional to the records
 * runs on the device (lofreq_amd/csrc/lfq_bamidx.hip), the merging of bins and the fill of the linear index on the host; device
 * memory is O(records + blocks).
 * `body` (the records' bytes) may lie inside the context's live lfq_bam_frame_encoded result or its live lfq_bgzf_inflate result:
 * the records are then taken from the device copy (n_from_device = 1); otherwise they go down once, through a pinned staging area
 * if the memory is pageable.  No other result of the context is invalidated: frame, encode, inflate and deflate results stay live.
 * LFQ_ERR_INVALID with *out = NULL.  Before a device is touched: a NULL argument, a negative count or file_off; rec_off or
 * comp_off not strictly increasing, data_off decreasing; [rec_off[0], rec_off[n_recs]) outside [data_off[0], data_off[n_blocks]]
 * or outside [0, n_bytes).  From the record pass, which reports the FIRST such record in lfq_bam_index_times.first_bad_record:
 * a record whose block_size + 4 is not rec_off[j + 1] - rec_off[j], or is below 36; l_read_name + 4 n_cigar_op above what is
 * left of it; refID >= n_ref or < -1; with refID >= 0, pos < -1 or an end above 2^29; records not sorted -- a refID >= 0 behind a
 * larger one or behind a refID < 0, or pos going down inside a reference.
 * n_recs == 0: LFQ_OK, an index of n_ref empty references, nothing launched.
 * *out is the CALLER'S, a host object with no tie to the context: free it with lfq_bam_index_free.  Blocks. */
typedef struct lfq_bam_index lfq_bam_index;
int lfq_bam_index_build(lfq_ctx *ctx, const uint8_t *body, int64_t n_bytes, const int64_t *rec_off, int64_t n_recs,
                        const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks, int64_t file_off, int32_t n_ref,
                        lfq_bam_index **out);
/* the context's last lfq_bam_index_build: records and tables down, the four kernels, the lists back -- on the device's clock --
 * and the host's finishing pass on the wall clock; first_bad_record: -1, or the record LFQ_ERR_INVALID was returned for */
typedef struct lfq_bam_index_times {
    double upload_ms, kernels_ms, download_ms, host_ms;
    int64_t n_recs, n_chunks, n_intervals, first_bad_record;
    int n_launches, n_from_device;
} lfq_bam_index_times;
int lfq_last_bam_index_times(lfq_ctx *ctx, lfq_bam_index_times *t);
/* Host only, no context.  The .bai: "BAI\1", n_ref; per reference n_bin, the bins in ascending number with 37450 last (bin,
 * n_chunk, chunks), n_intv, the offsets; n_no_coor.  *bai is idx's, valid until lfq_bam_index_free.  The binary writes the same
 * bins in its hash table's order: compare parsed files, not bytes. */
int lfq_bam_index_bytes(const lfq_bam_index *idx, const uint8_t **bai, int64_t *n_bytes);
/* any writer's .bai: bins in any order, the trailing n_no_coor optional.  LFQ_ERR_INVALID (*out = NULL): a NULL argument, no
 * magic, a count that runs past n_bytes, a bin twice in a reference, a bin above 37450, a pseudo-bin without exactly two
 * chunks, bytes left over. */
int lfq_bam_index_parse(const uint8_t *bai, int64_t n_bytes, lfq_bam_index **out);
/* the chunks of the file that hold every mapped record of reference tid overlapping [beg, end) (0-based, half-open): those of
 * the bins reg2bins(beg, end) names that end above the linear index's value for beg >> 14 (0 past n_intv), begun no earlier than
 * that value, sorted by begin, overlapping or touching ones merged.  The exact list is the library's own; its contract is that
 * every such record starts inside one of the chunks, that the chunks are sorted and disjoint and that none begins in front of the
 * linear value.  (A placed unmapped read is in its bin but not in the linear index, as in the binary: no query promises it.)  A
 * reference without records or an empty region: n_chunks = 0, LFQ_OK.  LFQ_ERR_INVALID: a NULL argument, tid outside
 * [0, n_ref).  The arrays are idx's, valid until its next query (an index is not to be queried from two threads at once). */
int lfq_bam_index_query(const lfq_bam_index *idx, int32_t tid, int64_t beg, int64_t end, const uint64_t **chunk_beg,
                        const uint64_t **chunk_end, int64_t *n_chunks);
void lfq_bam_index_free(lfq_bam_index *idx);
/* Host only: the two loops a writer runs between lfq_bam_frame_encoded / its own records and lfq_bgzf_deflate.
 * lfq_bam_record_chain: the offsets of EVERY complete record of bam[first .. stop), none filtered (lfq_bam_scan_records filters):
 * rec_off[n_recs] is where the first incomplete record starts.  LFQ_ERR_INVALID: a NULL argument, first < 0, stop < first, a
 * block_size below 32.
 * lfq_bam_record_cuts: the cuts_or_null of lfq_bgzf_deflate for pieces of at most max_piece bytes of [rec_off[0],
 * rec_off[n_recs]), greedy: each cut is the last record boundary that keeps the piece that long; a record longer than max_piece
 * is cut every max_piece bytes.  LFQ_ERR_INVALID: a NULL argument, n_recs < 0, max_piece <= 0, rec_off not increasing. */
int lfq_bam_record_chain(const uint8_t *bam, int64_t first, int64_t stop, int64_t **rec_off, int64_t *n_recs);
void lfq_bam_record_chain_free(int64_t *rec_off);
int lfq_bam_record_cuts(const int64_t *rec_off, int64_t n_recs, int64_t max_piece, int64_t **cuts, int64_t *n_cuts);
void lfq_bam_record_cuts_free(int64_t *cuts);

/* --- source quality: the per-read pre-step of `lofreq call -s` -------------------------
 * source_qual (plp.c:427-593) over count_cigar_ops (samutils.c:437-614) for a batch of reads of one contig (same
 * read layout as lfq_baq_batch; the reference letters are compared as given, the caller upper-cases the contig
 * like mplp_func does, plp.c:652).  def_nm_q: -T/--def-nm-q (>= 0 replaces EVERY operation's quality, :500-504;
 * -1 = off); min_bq: the reference passes DEFAULT_MIN_BQ = 6 (plp.c:728); ign_or_null: one byte per reference
 * position, != 0 where the -S/--ign-vcf list has a variant (var_in_ign_list, plp.c:305-323).
 * sq_out[r] = what source_qual returns: -1 (nothing to count), 49314 (at most one non-match) or
 * (int)(-10 log10l(1 - P)) (INT32_MIN when P rounds to 1, as the x86-64 build yields); mplp_func stores
 * max(sq, 0) in the read's `sq` tag (plp.c:731-734).  sq_byte_or_null[r] gets the byte the packed sq track takes:
 * min(max(sq, 0), 254) -- every value above 3240 is the probability 0.0 in PHREDQUAL_TO_PROB, and source_qual
 * yields nothing between 160 and 49314. */
int lfq_source_qual_batch(lfq_ctx *ctx, const lfq_baq_reads *reads, int def_nm_q, int min_bq,
                          const uint8_t *ign_or_null, int32_t *sq_out, uint8_t *sq_byte_or_null);

/* Strand counts (ref_fw / ref_rv / alt_fw) and the unfiltered alt counts (alt_raw_counts, the AF numerator) are only ever
 * read for reported variants (DP4, SB and AF: lofreq_call.c:117-129, 835, 853-857), and counting them for every column
 * costs the dominant kernel half of its instructions.  With on = 0, lfq_snv_batch_device and lfq_call_snvs_submit
 * count them only for the columns of the sparse output (lfq_col_pvals.counts is complete either way, and so are the
 * records); in the dense lfq_col_counts entries the strand fields are then 0 and alt_raw_counts is either the true
 * value or 0 (which kernel ran decides; the decision fields n_err_probs, alt_counts, kmax, tested, gated, coverage are
 * always there).  Default: on = 1.  lfq_call_snvs_batch decides by itself: complete dense entries exactly when
 * h_counts_or_null is given. */
int lfq_set_dense_strand_counts(lfq_ctx *ctx, int on);

/* One step further for a caller of lfq_snv_batch_device that reads only the sparse output: with on = 0 the dense entry of a
 * column that is not tested (tested == 0: nothing downstream looks at it) need not be written at all -- d_counts then keeps
 * whatever it held there (the shared-wavefront count kernel, i.e. batches of the packed nt layout whose deepest column has at
 * most a few thousand observations, skips those stores; at 200x the dense entries are a fifth of the bytes it moves, at the
 * price HBM asks for writes among reads).  Takes effect only together with lfq_set_dense_strand_counts(ctx, 0).
 * Default: on = 1.  (lfq_call_snvs_batch without h_counts runs this way by itself on the context's own array;
 * lfq_call_snvs_submit only after lfq_set_dense_counts(ctx, 0), and lfq_call_snvs_collect then refuses h_counts.) */
int lfq_set_dense_counts(lfq_ctx *ctx, int on);

/* The profile HMM's gap-open and gap-extension probabilities, kpa_ext_par_t.d / .e (kprobaln_ext.h:31-34), for every
 * BAQ call of the context after this one.  Default: kpa_ext_par_lofreq_illumina = { 1e-5, 0.4 } (kprobaln_ext.c:50), what
 * bam_prob_realn_core_ext uses (bam_md_ext.c:275); a reference built with -DPACBIO_REALN uses kpa_ext_par_lofreq_pacbio =
 * { 0.1, 0.4 } (kprobaln_ext.c:51, bam_md_ext.c:268-273).  kpa_ext_par_t.bw is not a parameter: the caller overwrites it
 * per read (bam_md_ext.c:376-379).  0 < gap_open < 0.5, 0 < gap_ext < 1, else LFQ_ERR_INVALID. */
int lfq_set_baq_hmm_params(lfq_ctx *ctx, float gap_open, float gap_ext);

/* nt layout of the tracks the device pileup returns: on = 1 (default) LFQ_TRACKS_NT_PACKED, on = 0 one byte per
 * observation.  lfq_pack_nt_track: the same packing for a host byte track (packed_out: (n_obs + 7) / 8 * 4 bytes). */
int lfq_set_pileup_nt_packed(lfq_ctx *ctx, int on);
/* Reads that are NOT sorted by position: off (default) = the pileup calls return LFQ_ERR_INVALID, as mpileup stops at a file
 * that is not coordinate-sorted (bam_mplp_auto, plp.c:1406-1447); on = they are taken by the read-major kernels (one thread per
 * read, an atomic cursor per column): the same columns and the same observations per column, but in no fixed ORDER within a
 * column, so that the last bits of a p-value can differ from run to run (QUAL and every integer output do not). */
int lfq_set_pileup_unsorted(lfq_ctx *ctx, int on);
/* -d / --max-depth of `lofreq call` (mplp_conf_t.max_depth, plp.c:120, set with bam_mplp_set_maxcnt, plp.c:1391-1392) for
 * the read-level pileups of this context: lfq_readset_pileup_snv / _indels and lfq_pileup_snv_tracks / lfq_pileup_indel_columns.
 * It is htslib's rule (bam_plp_push), not a per-column clamp.  On the reads in file order: the first read that starts at a
 * position P is always kept; every later read at P is dropped if at least max_depth of the KEPT reads before it reach P
 * (exclusive end >= P: a read whose last base is P - 1 still counts).  A dropped read is in no column: a position covered by
 * dropped reads only is no column at all.  Unsorted reads with a cap are LFQ_ERR_INVALID (the rule is defined on file order).
 * LFQ_NO_MAX_DEPTH (the default): no cap, the pileups as without this call.  Not reproduced (htslib details no caller needs):
 * with max_depth = 0 htslib drops the very first read of contig 0 when it starts at position 0.  A negative -d keeps only the
 * first read of each start position in htslib, which is max_depth = 0 here: callers map it, because -1 (LFQ_NO_MAX_DEPTH) means
 * no cap and every value below it is LFQ_ERR_INVALID. */
#define LFQ_NO_MAX_DEPTH (-1)
int lfq_set_max_depth(lfq_ctx *ctx, int64_t max_depth);
int lfq_pack_nt_track(const uint8_t *nt_bytes, int64_t n_obs, uint8_t *packed_out);

/* ---- -l / --bed of `lofreq call`: the targets (bedidx.c) ------------------------------------------------------------------------
 * lfq_bed_parse reads BED text that is already decompressed (gzip stays with the caller) by the rules of bed_read, line by line:
 *   - an EMPTY line ends the text silently, everything behind it is ignored (the reference's read loop stops at a line of length
 *     0); a line of blanks only and a line whose first non-blank is '#' are skipped; a trailing '\r' is a blank;
 *   - leading blanks are stripped, the name runs to the next blank, the rest is sscanf("%u %u"): two numbers are the BED interval
 *     [beg, end), one number is the 1-based position list format, [p - 1, p) ("c1 100 rs5" and "c1 100.5 102" are position 100; a
 *     leading '+' is accepted);
 *   - refused, with the whole text (LFQ_ERR_INVALID, *bad_line_or_null = the 1-based line): no number, unless the name is `browser`
 *     or `track` (skipped); end < beg after the conversion ("c1 0" of the list format, "c1 -5 7"); and, a departure from the
 *     reference, which compares such values as negative ints: a value above INT32_MAX;
 *   - beg == end is accepted; the lines of one name are pooled wherever they stand; duplicates and overlaps are kept.
 * The table of a name is sorted by (beg, end).  lfq_bed_overlap is bed_overlap's predicate: 1 iff some interval of the name has
 * end_i > beg and beg_i < end, 0 for a name the BED does not hold.  A zero-length interval [x, x) therefore matches a read with
 * pos < x < endpos and never a column.  No context, no device. */
typedef struct lfq_bed lfq_bed;
int lfq_bed_parse(const char *text, int64_t n_bytes, lfq_bed **bed_out, int64_t *bad_line_or_null);
void lfq_bed_free(lfq_bed *bed);
int64_t lfq_bed_n_names(const lfq_bed *bed);
const char *lfq_bed_name(const lfq_bed *bed, int64_t i);          /* in order of first appearance; NULL outside [0, n_names) */
/* the intervals of `name` in sorted order: *beg_out / *end_out point into the BED (valid until lfq_bed_free), *n_out = how many;
 * a name the BED does not hold: LFQ_OK, *n_out = 0, both pointers NULL */
int lfq_bed_intervals(const lfq_bed *bed, const char *name, const int32_t **beg_out, const int32_t **end_out, int64_t *n_out);
int lfq_bed_overlap(const lfq_bed *bed, const char *name, int64_t beg, int64_t end);     /* 0 / 1; NULL arguments: 0 */

/* The targets of the read-level pileups of this context.  The table of `name` goes to the device and the context keeps its own copy:
 * the caller may free the BED at once.  bed_or_null = NULL takes the targets off again (name is then ignored).  A name the BED does
 * not hold is an empty table: nothing overlaps, no read and no column.
 * A READ SET TAKES THE CONTEXT'S TARGETS WHEN IT IS CREATED (every lfq_readset_create*, and the read set lfq_readset_viterbi makes);
 * a later lfq_set_bed changes the read sets created after it only, so that BAQ, the kept reads and both pileups of one read set
 * see one BED.  For such a read set, as `lofreq call -l` does it:
 *   - reads (plp.c:625-629): a read whose [pos, bam_endpos) overlaps no interval is dropped before BAQ and before the -d cap.
 *     lfq_readset_baq / _baq_fill launch the HMM for the other reads only (lfq_last_baq_times.n_reads counts those; a dropped
 *     read keeps lb 0, ai / ad '~' and tag_flags 0), lfq_set_max_depth's rule runs on the survivors in file order, and
 *     lfq_readset_kept_reads reports BED and cap together.  Unsorted reads (lfq_set_pileup_unsorted) are taken with a BED alone
 *     and stay LFQ_ERR_INVALID with a cap;
 *   - columns (plp.c:1412): lfq_readset_pileup_snv, lfq_readset_pileup_indels and lfq_readset_plp_summary hand out the covered
 *     positions p whose [p, p + 1) overlaps an interval, in one column numbering.  The decision is made on the device, on the
 *     per-position counters of the count pass.
 * lfq_readset_pileup_sites and lfq_readset_uniq take every read (`lofreq uniq` has no -l); lfq_readset_source_qual and
 * lfq_readset_indelqual compute their values for every read.
 * LFQ_ERR_INVALID: ctx NULL, or bed given and name NULL. */
int lfq_set_bed(lfq_ctx *ctx, const lfq_bed *bed_or_null, const char *name_or_null);

/* ---- `lofreq faidx`, the contig in front of every region, `lofreq checkref` ----------------------------------------------------------
 * The `ref` every read-level entry takes (lfq_baq_reads.ref, lfq_pileup_reads.ref, lfq_bam_records.ref) is a whole contig of a FASTA:
 * faidx_fetch_seq(fai, name, 0, 0x7fffffff, &len).  These functions make the index (`lofreq faidx`, fai_build) and the contig on the
 * device from the file's bytes, by the rules of the 2.1.4 binary (lofreq_amd/csrc/lfq_fasta.h states them):
 *   - a line is a header iff its first byte is '>'; its name: the bytes behind '>' after leading blanks up to the next blank (may be
 *     empty); .fai line: name, length, offset, line_blen, line_len, tab-separated;
 *   - length counts the graph bytes (0x21 .. 0x7e) of the sequence's lines, line_blen / line_len are the first line's graph bytes and
 *     its bytes with the terminator ("\r" counts towards line_len only); a last line without '\n' counts as if it had one;
 *   - a line with more BYTES than line_len: refused, LFQ_FASTA_LINE_LENGTH.  A line with fewer (the empty line too) ends the sequence,
 *     and only "\n" and "\r\n" lines may follow before the next header; anything else, and any other text in front of the first
 *     header: LFQ_FASTA_UNEXPECTED.  *bad_line is the 1-based line, *bad_byte the byte htslib's message shows (the line's first, or the
 *     one behind a leading '\r'; -1: the file ends there);
 *   - a header followed by an empty line, another header or nothing has no sequence: dropped silently in mid-file; the whole file is
 *     refused when it is the LAST header (LFQ_FASTA_LAST_EMPTY).  A file without any header: LFQ_FASTA_EMPTY_FILE;
 *   - of equal names the first stays (lfq_fasta_index_n_duplicates counts the others).
 * Only whole contigs are fetched, as the reference does; FASTQ is not read; files are the caller's to read.
 *
 * lfq_fasta_open uploads the bytes (device to device when they lie inside the context's live lfq_bgzf_inflate result -- a bgzip-
 * compressed FASTA --, lfq_fasta_times.n_from_device says so) and scans them; the file stays resident until lfq_fasta_close, which must
 * come before lfq_destroy.  The caller's bytes are not needed after the call.  n_bytes == 0 is LFQ_OK: the index build then refuses.
 * LFQ_ERR_INVALID: ctx / out NULL, n_bytes < 0, bytes NULL with n_bytes > 0.  Blocks. */
typedef struct lfq_fasta lfq_fasta;
typedef struct lfq_fasta_index lfq_fasta_index;
#define LFQ_FASTA_OK 0
#define LFQ_FASTA_UNEXPECTED 1
#define LFQ_FASTA_LINE_LENGTH 2
#define LFQ_FASTA_LAST_EMPTY 3
#define LFQ_FASTA_EMPTY_FILE 4
int lfq_fasta_open(lfq_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, lfq_fasta **out);
void lfq_fasta_close(lfq_fasta *fa);
/* the index of the resident file.  LFQ_OK and *out (the caller's, lfq_fasta_index_free), or LFQ_ERR_INVALID with *why_or_null one of
 * LFQ_FASTA_* and the place of the FIRST offending line (found by an atomic minimum over the lines: the same on every run).  Blocks. */
int lfq_fasta_index_build(lfq_fasta *fa, lfq_fasta_index **out, int *why_or_null, int64_t *bad_line_or_null, int *bad_byte_or_null);
/* host only, no context.  The .fai text of an index (the index's, valid until it is freed) and an index from .fai text -- one the
 * caller read from disk, possibly made by another tool for another version of the file.  Columns behind the fifth are ignored;
 * LFQ_ERR_INVALID: fewer than five columns in a line, a column that is no non-negative decimal number */
int lfq_fasta_index_text(const lfq_fasta_index *idx, const char **text, int64_t *n_bytes);
int lfq_fasta_index_parse(const char *text, int64_t n_bytes, lfq_fasta_index **out);
void lfq_fasta_index_free(lfq_fasta_index *idx);
typedef struct lfq_fasta_entry {
    int64_t length, offset;
    int32_t line_blen, line_len;
} lfq_fasta_entry;
int64_t lfq_fasta_index_n(const lfq_fasta_index *idx);
int64_t lfq_fasta_index_n_duplicates(const lfq_fasta_index *idx);
const char *lfq_fasta_index_name(const lfq_fasta_index *idx, int64_t i);     /* in file order; NULL outside [0, n) */
int lfq_fasta_index_entry(const lfq_fasta_index *idx, int64_t i, lfq_fasta_entry *entry);
int64_t lfq_fasta_index_find(const lfq_fasta_index *idx, const char *name); /* -1: no such name */
/* The whole contig `name`: the `length` graph bytes at or behind `offset`, in file order, case kept (every consumer of `ref` upper-
 * cases for itself).  seq is pinned host memory with a NUL behind it, d_seq the same bytes on the device; both are the file's, valid
 * until the next lfq_fasta_fetch on it or lfq_fasta_close.  WHILE IT IS VALID, a `ref` pointer inside [seq, seq + len) given to
 * lfq_readset_create* on this context is copied device to device instead of across the link (lfq_readset_ref_from_device).
 * The index may be a parsed one.  Its entry is checked before anything is launched: LFQ_ERR_INVALID when the name is not in the index,
 * offset lies outside [0, n_bytes] or fewer than `length` graph bytes stand behind it.  Two kernels serve: LFQ_FASTA_PATH_REGULAR
 * (base p from offset + p / line_blen * line_len + p % line_blen) only after a launch has proved from the line records that every line
 * of the span but the last is line_blen graph bytes and '\n'; LFQ_FASTA_PATH_GENERAL (by graph rank) for everything else: blanks inside
 * lines, "\r\n", an index that does not describe the file.  Blocks. */
typedef struct lfq_fasta_contig {
    const uint8_t *seq;
    int64_t len;
    const uint8_t *d_seq;
} lfq_fasta_contig;
int lfq_fasta_fetch(lfq_fasta *fa, const lfq_fasta_index *idx, const char *name, const lfq_fasta_contig **out);
#define LFQ_FASTA_PATH_NONE 0       /* nothing fetched yet, or a contig of length 0 */
#define LFQ_FASTA_PATH_REGULAR 1
#define LFQ_FASTA_PATH_GENERAL 2
/* the context's last lfq_fasta_open and what followed it: upload and download on the host's clock, the kernels on the device's.
 * n_handovers: contigs read sets took from a live fetch result since that open */
typedef struct lfq_fasta_times {
    double upload_ms, scan_ms, lines_ms, fetch_ms, download_ms;
    int64_t n_bytes, n_lines, n_headers, n_fetch_bytes;
    int n_launches, n_from_device, fetch_path, n_handovers;
} lfq_fasta_times;
int lfq_last_fasta_times(lfq_ctx *ctx, lfq_fasta_times *t);
int lfq_readset_ref_from_device(const lfq_readset *rs);     /* 1: this read set's contig came from a live fetch result */
/* `lofreq checkref` (samutils.c:621-676; plp.c:1416 applies the same test): per @SQ of a BAM header, in order, the name must be in the
 * index and the lengths equal.  The first failure ends it: *first_bad is its position (-1: none), *why says which.  Host only; the
 * header's parse is the caller's.  LFQ_ERR_INVALID: idx NULL, n < 0, names / lens NULL with n > 0 */
#define LFQ_CHECKREF_OK 0
#define LFQ_CHECKREF_NO_SEQUENCE 1
#define LFQ_CHECKREF_LENGTH 2
int lfq_checkref(const lfq_fasta_index *idx, const char *const *names, const int64_t *lens, int64_t n, int64_t *first_bad_or_null,
                 int *why_or_null);
/* The .gzi `lofreq faidx` writes beside a bgzip-compressed FASTA, from the block tables of an lfq_bgzf_inflate result: a little-endian
 * uint64 count, then per block with data behind the first such one the pair (compressed offset of the first block behind the previous
 * block with data -- empty blocks in between belong to it --, uncompressed offset of the block).  *n_bytes is its size;
 * out NULL: only that.  Host only.  LFQ_ERR_INVALID: res / n_bytes NULL, capacity below *n_bytes */
int lfq_bgzf_gzi_bytes(const lfq_bgzf_result *res, uint8_t *out_or_null, int64_t capacity, int64_t *n_bytes);

/* ---- VCF text, parsed on the device, and `lofreq vcfset` -------------------------------------------------------------------------------
 * (ABI version 10 still: new functions, new structs, a new opaque type; no existing layout changed.)
 * lfq_vcf_open keeps the bytes of an UNCOMPRESSED VCF resident (device to device when they lie inside the context's live
 * lfq_bgzf_inflate result -- a bgzipped VCF is inflated first --, lfq_vcf_times.n_from_device says so) and parses them by the rules of the
 * 2.1.4 binary (lofreq_amd/csrc/lfq_vcf.h states them with their places in vcf.c):
 *   LFQ_VCF_STREAM  as vcf_parse_header / vcf_parse_var read a file: the header is every line up to and including the first, among the
 *                   first 10 000, whose first 38 bytes are "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"; the records start behind it, or
 *                   at line 1 when there is none ('#' lines are records then); they END silently at the first line with fewer than five
 *                   tab-separated fields (lfq_vcf_n_lines_behind counts that line and what follows).
 *   LFQ_VCF_TABIX   as the second file of vcfset is read through its index: '#' lines are skipped anywhere; refused: a line with fewer
 *                   than five fields (LFQ_VCF_FIELDS), a CHROM in two runs or a POS below the one before it in its run
 *                   (LFQ_VCF_UNSORTED), POS < 1, an empty REF, an INFO END= below POS (LFQ_VCF_INTERVAL).
 *   both            pos = atol(POS) - 1, qual = atoi(QUAL) or -1 for '.' / no QUAL; fewer than eight fields: FILTER and INFO are ".".
 *                   Refused, departures from the reference: a line of more than 8 190 bytes (an fgets into vcf.c's LINE_BUF_SIZE 8192 would split it; THE 2.1.4 BINARY was built with
 *                   half that buffer and already splits a line behind 4 095 bytes, silently: lines of 4 096 .. 8 190 bytes are read whole here;
 *                   LFQ_VCF_LINE_TOO_LONG), a NUL byte (LFQ_VCF_NUL), more than 18 digits in POS or 9 in QUAL (LFQ_VCF_NUMBER).
 * A refusal is LFQ_ERR_INVALID with *why_or_null and the 1-based line of the FIRST offending line (the smallest line, then the smallest
 * reason: the same on every run).  n_bytes == 0: LFQ_OK, no records, nothing launched.  LFQ_ERR_INVALID before a device is touched: ctx /
 * out NULL, n_bytes < 0, bytes NULL with n_bytes > 0, an unknown mode.  Blocks.  lfq_vcf_close must come before lfq_destroy. */
typedef struct lfq_vcf lfq_vcf;
typedef struct lfq_filter_var lfq_filter_var;           /* (both defined further down) */
typedef struct lfq_uniq_variants lfq_uniq_variants;
#define LFQ_VCF_STREAM 0
#define LFQ_VCF_TABIX 1
#define LFQ_VCF_OK 0
#define LFQ_VCF_LINE_TOO_LONG 1
#define LFQ_VCF_NUL 2
#define LFQ_VCF_NUMBER 3
#define LFQ_VCF_FIELDS 4
#define LFQ_VCF_UNSORTED 5
#define LFQ_VCF_INTERVAL 6
#define LFQ_VCF_MULTIALLELIC 7
int lfq_vcf_open(lfq_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, int mode, lfq_vcf **out, int *why_or_null, int64_t *bad_line_or_null);
void lfq_vcf_close(lfq_vcf *vcf);
int64_t lfq_vcf_n_records(const lfq_vcf *vcf);
int64_t lfq_vcf_n_lines_behind(const lfq_vcf *vcf);
/* the header's text (the file's own, valid until close; empty when *found = 0 -- the callers then write their default header) */
int lfq_vcf_header(lfq_vcf *vcf, const char **text, int64_t *n_bytes, int *found);
/* bits of flags[] */
#define LFQ_VCF_F_PASSES 1u         /* VCF_VAR_PASSES (vcf.h:87), a PREFIX rule: FILTER starts with '.' or with "PASS" */
#define LFQ_VCF_F_FILTERED 2u       /* vcf_var_filtered (vcf.c:315-326), an EXACT rule: FILTER is neither "." nor "PASS" */
#define LFQ_VCF_F_INDEL_LEN 4u      /* strlen(REF) > 1 || strlen(ALT) > 1 */
#define LFQ_VCF_F_INDEL_KEY 8u      /* INFO has the key INDEL (vcf_var_has_info_key: case-insensitive, '=' or the token's end) */
#define LFQ_VCF_F_ALT_COMMA 16u
/* host copies of the record table (the file's own, made on the first call, valid until close).  Record r is line line[r] (0-based);
 * field j (0-based, j < n_fields[r], which is capped at 10: 9 = FORMAT alone, 10 = samples behind it; offsets exist for fields 1 - 9) starts field_off[10 r + j] bytes
 * behind line_start[line[r]] and ends one byte in front of the next field; field_off[10 r + 9] is the line's end after chomp.
 * run_id[r]: the run of equal CHROM strings the record stands in; run_name[i], run_begin[i] .. run_begin[i + 1]: its name and records */
typedef struct lfq_vcf_table {
    int64_t n_records, n_lines, n_runs;
    const int64_t *line, *line_start, *pos;
    const int32_t *qual;
    const uint8_t *flags, *n_fields;
    const uint16_t *field_off;
    const int32_t *run_id;
    const int64_t *run_begin;
    const char *const *run_name;
} lfq_vcf_table;
int lfq_vcf_records(lfq_vcf *vcf, lfq_vcf_table *out);
/* out[n_records], ready for lfq_filter_vars: is_indel = vcf_var_is_indel, qual, dp / sb by strtol / atoi of INFO DP / SB (0 where the key
 * is missing), alt_fw / alt_rv from DP4 (-1 unless it has exactly four fields, vcf.c:566-604), af = the C library's strtof on the bytes
 * of AF's value, which the device located (0 where missing) */
int lfq_vcf_filter_vars(lfq_vcf *vcf, lfq_filter_var *out);
/* the variants of CHROM `chrom` as `lofreq uniq` reads them (lofreq_uniq.c:684: with only_unfiltered, those vcf_var_filtered lets
 * through), ready for lfq_readset_uniq; af = uni_freq when that is > 0, else strtof of AF -- a record without AF is then
 * LFQ_ERR_INVALID with *bad_line_or_null its 1-based line (lofreq_uniq.c:257-261).  (*line_of_variant)[i]: the 0-based line of variant i.
 * The arrays are the file's own, valid until the next call on it or close */
int lfq_vcf_uniq_variants(lfq_vcf *vcf, const char *chrom, int only_unfiltered, float uni_freq, lfq_uniq_variants *out,
                          int64_t **line_of_variant, int64_t *bad_line_or_null);
/* -S / --ign-vcf (source_qual_load_ign_vcf, plp.c:337-399): mask[pos] |= 1 for every record of `chrom` with 0 <= pos < ref_len, under a
 * BED only where [pos, pos + 1) overlaps its table of that name (plp.c:376).  ORs into the caller's array, so several files accumulate
 * (lofreq_call.c:1453-1463); the result is what lfq_source_qual_batch and lfq_readset_source_qual take as ign_or_null */
int lfq_vcf_ign_mask(lfq_vcf *vcf, const char *chrom, int64_t ref_len, const lfq_bed *bed_or_null, uint8_t *mask);
/* `lofreq vcfset` (lofreq_vcfset.c): intersect / complement of vcf1 (stream mode) against vcf2 (tabix mode), or concat of vcf1 and
 * more[0 .. n_more) (stream mode; their headers are skipped, no matching).  Per record of vcf1, in the reference's order (:387-411):
 * --only-snvs / --only-indels drop it silently; then a ',' in ALT without --only-pos refuses the whole call (LFQ_VCF_MULTIALLELIC);
 * then --only-passed (VCF_VAR_PASSES) skips it and counts it in n_ignored.  A candidate of vcf2 has the same CHROM string and the same
 * POS, passes the same three filters (:452-477) and, without --only-pos, has bytewise the same REF and ALT.  A record of vcf1 with
 * POS < 1 that reaches the match is refused (LFQ_VCF_INTERVAL).  The lines are WRITTEN, not copied (vcf_write_var, vcf.c:469-497): POS
 * and QUAL from the parsed values, FILTER / INFO "." for short lines, add_info_or_null appended by vcf_var_add_to_info's rule.
 * The result is the context's own, valid until its next lfq_vcfset: keep[n_keep] has LFQ_VCFSET_* per record (of every file in turn
 * for concat), text (pinned memory) is vcf1's header, if found, and the lines; with count_only no text is made.
 * LFQ_ERR_INVALID before a device is touched: a NULL vcf1 / conf / out, an unknown op, only_snvs && only_indels, no vcf2 or n_more > 0
 * for intersect / complement, n_more < 0, files of different contexts.  A refusal is LFQ_ERR_INVALID with *out set and why, bad_file
 * (0 = vcf1, i + 1 = more[i]) and bad_line filled in.  Blocks. */
#define LFQ_VCFSET_INTERSECT 0
#define LFQ_VCFSET_COMPLEMENT 1
#define LFQ_VCFSET_CONCAT 2
#define LFQ_VCFSET_DROPPED 0
#define LFQ_VCFSET_IGNORED 1
#define LFQ_VCFSET_TAKEN 2          /* counted in n_vars1, not written */
#define LFQ_VCFSET_WRITTEN 3
typedef struct lfq_vcfset_conf {
    int op, only_passed, only_pos, only_snvs, only_indels, count_only;
    const char *add_info_or_null;
} lfq_vcfset_conf;
typedef struct lfq_vcfset_result {
    int64_t n_vars1, n_ignored, n_out, n_keep;
    const uint8_t *keep;
    const char *text;
    int64_t text_bytes;
    int64_t bad_line;
    int why, bad_file;
} lfq_vcfset_result;
int lfq_vcfset(lfq_vcf *vcf1, lfq_vcf *vcf2_or_null, lfq_vcf *const *more, int64_t n_more, const lfq_vcfset_conf *conf,
               const lfq_vcfset_result **out);
/* the context's last lfq_vcf_open and what followed it on that context: the kernels on the device's clock, both link legs on the host's.
 * n_launches counts every launch since that open, n_set_launches those of the last lfq_vcfset */
typedef struct lfq_vcf_times {
    double upload_ms, scan_ms, parse_ms, info_ms, match_ms, emit_ms, download_ms;
    int64_t n_bytes, n_lines, n_records;
    int n_launches, n_from_device, n_set_launches, pad_;
} lfq_vcf_times;
int lfq_last_vcf_times(lfq_ctx *ctx, lfq_vcf_times *t);

/* ---- the index of a bgzipped VCF: its .tbi built on the device, written, read, queried, and a region opened through it ---------------
 * (ABI version 10 still: new functions, a new struct, a new opaque type; no existing layout changed.)
 * lfq_vcf_index_build makes the tabix index of a file opened in LFQ_VCF_TABIX mode whose text lies in BGZF blocks with the tables
 * data_off / comp_off ([n_blocks + 1] each, as lfq_bgzf_deflated and lfq_bgzf_result give them; data_off[0] = 0, data_off[n_blocks] =
 * the text's length): block b holds the text's bytes [data_off[b], data_off[b + 1]) and starts at byte comp_off[b] + file_off of the
 * .vcf.gz; empty blocks at the tables' end (the end-of-file marker an lfq_bgzf_result lists) are dropped, so that the text ends where the
 * marker starts.  The index is the one the reference's 2.1.4 binary writes beside every .vcf.gz (vcf_file_close, vcf.c:256-270), name for
 * name, bin for bin and chunk for chunk; lofreq_amd/csrc/lfq_tbx.h states the rules, INTEGRATION.md section 14 lists them and
 * tests/golden/tbi_binary.json holds them to the binary: a record's interval is [POS - 1, END= value, or POS - 1 + len(REF)), its
 * chunk begins where the record in front of it ends ('#' lines between two records therefore belong to the second one's chunk) and
 * the last record's ends at the text's end.  One lane per record reads the table the open left on the device (the text is neither
 * uploaded nor read again, except for END= values), then lfq_bam_index_build's own compaction kernels and host pass run: four launches
 * whatever the record count, device memory O(records + blocks).
 * Refused with LFQ_ERR_INVALID, *why_or_null = LFQ_VCF_RANGE and the 1-based FIRST such line: an interval a .tbi cannot hold -- an end
 * above 2^29 (POS 2^29 is taken, POS 2^29 + 1 and END=2^29 + 1 are not; the binary then writes no index), or an END= of more than 18
 * digits.  LFQ_ERR_INVALID before a launch: a NULL vcf / out / table, a file opened in stream mode, a negative n_blocks or file_off,
 * comp_off not strictly increasing or negative, data_off decreasing, data_off[0] != 0, data_off[n_blocks] != the text's length.
 * A file without records: LFQ_OK, an index of no names (as the binary's .tbi of a header-only file), nothing launched.
 * No result of the context is invalidated.  *out is the CALLER'S, a host object with no tie to the context or the file: free it with
 * lfq_vcf_index_free.  Blocks.
 * The cuts of lfq_bgzf_deflate that keep lines whole -- the binary's blocks end on line boundaries -- are what lfq_bam_record_cuts gives
 * for rec_off = the table's line_start[0 .. n_lines) followed by the text's length: no function of their own. */
#define LFQ_VCF_RANGE 8
typedef struct lfq_vcf_index lfq_vcf_index;
int lfq_vcf_index_build(lfq_vcf *vcf, const int64_t *data_off, const int64_t *comp_off, int64_t n_blocks, int64_t file_off,
                        lfq_vcf_index **out, int *why_or_null, int64_t *bad_line_or_null);
/* the last lfq_vcf_index_build on the context of its file: the four kernels and the lists' way back on the device's clock, the host's
 * finishing pass on the wall clock */
typedef struct lfq_vcf_index_times {
    double kernels_ms, download_ms, host_ms;
    int64_t n_records, n_chunks, n_intervals;
    int n_launches, pad_;
} lfq_vcf_index_times;
int lfq_last_vcf_index_times(lfq_ctx *ctx, lfq_vcf_index_times *t);
/* Host only, no context.  The UNCOMPRESSED .tbi (on disk it is BGZF-compressed: lfq_bgzf_deflate with LFQ_BGZF_PUT_EOF, lfq_bgzf_inflate):
 * "TBI\1", n_ref, format (2), col_seq (1), col_beg (2), col_end (0), meta ('#'), skip (0), l_nm, the names NUL-terminated, then per name
 * what a .bai holds per reference (lfq_bam_index_bytes) and n_no_coor (0).  *tbi is idx's, valid until lfq_vcf_index_free. */
int lfq_vcf_index_bytes(const lfq_vcf_index *idx, const uint8_t **tbi, int64_t *n_bytes);
/* any writer's .tbi, inflated: bins in any order, the trailing n_no_coor optional; format, columns, meta and skip are kept and given back
 * by lfq_vcf_index_bytes.  LFQ_ERR_INVALID (*out = NULL): a NULL argument, no magic, a count that runs past n_bytes, l_nm that is not
 * exactly n_ref NUL-terminated names, a name twice, and everything lfq_bam_index_parse refuses of the rest. */
int lfq_vcf_index_parse(const uint8_t *tbi, int64_t n_bytes, lfq_vcf_index **out);
int64_t lfq_vcf_index_n_names(const lfq_vcf_index *idx);
const char *lfq_vcf_index_name(const lfq_vcf_index *idx, int64_t i);           /* idx's, NULL outside [0, n_names) */
/* the chunks that hold every record of `chrom` overlapping [beg, end) (0-based, half-open): by name, then lfq_bam_index_query's list
 * and contract -- every such record's line starts inside one of the chunks, they are sorted and disjoint, none begins in front of the
 * linear value.  A name the index lacks or an empty region: n_chunks = 0, LFQ_OK.  LFQ_ERR_INVALID: a NULL argument.  The arrays are
 * idx's, valid until its next query or lfq_vcf_open_indexed (an index is not to be queried from two threads at once). */
int lfq_vcf_index_query(const lfq_vcf_index *idx, const char *chrom, int64_t beg, int64_t end, const uint64_t **chunk_beg,
                        const uint64_t **chunk_end, int64_t *n_chunks);
void lfq_vcf_index_free(lfq_vcf_index *idx);
/* A region of a large second file (dbSNP for a viral contig): `comp` is the whole .vcf.gz as it lies on disk and idx its index.  The
 * index is queried; the BGZF blocks from the one the first chunk begins in to the one the last chunk ends in are inflated with
 * lfq_bgzf_inflate -- only that slice of comp goes down the link --; the bytes from the first chunk's begin to the last chunk's end are
 * opened in LFQ_VCF_TABIX mode, device to device.  Chunks begin and end on line boundaries, and a span of a sorted file is sorted with
 * one run per CHROM, so the result is a file like any other: it holds every record of `chrom` overlapping [beg, end), MAY HOLD MORE
 * (records in front of, behind and between them, of other names too) and never less.  No chunk: an open of zero bytes, nothing
 * inflated.  The call REPLACES the context's live lfq_bgzf_inflate result, as any inflate does.  why / bad_line as lfq_vcf_open, the
 * line counted from the span's first.  LFQ_ERR_INVALID before a device is touched: a NULL argument, n_comp < 0, chunks that lie outside
 * comp or not on its block boundaries (another file's index). */
int lfq_vcf_open_indexed(lfq_ctx *ctx, const uint8_t *comp, int64_t n_comp, const lfq_vcf_index *idx, const char *chrom, int64_t beg,
                         int64_t end, lfq_vcf **out, int *why_or_null, int64_t *bad_line_or_null);

/* lfq_call_snvs_batch in two halves, for callers that keep more than one batch in flight (one context per batch in
 * flight): submit launches the kernels and returns; collect waits, fetches the sparse records and finishes them on
 * the host.  While batch k is collected, the kernels of batch k+1 (submitted on another context) run.  conf's
 * running Bonferroni factor is read at submit and advanced at collect, so batches in flight at the same time
 * need confs of their own -- independent regions, as call-parallel's bins are.  Host tracks handed to submit
 * (tracks_on_device = 0) must stay valid until collect.  A second submit on a context whose batch has not been
 * collected returns LFQ_ERR_INVALID. */
int lfq_call_snvs_submit(lfq_ctx *ctx, const lfq_conf *conf, const lfq_tracks *tracks, int tracks_on_device);
/* blocks until the KERNELS of the submitted batch are done.  The pattern that keeps one GPU busy with two contexts:
 * wait(A); submit(B, next batch); collect(A) -- the host finish of batch k runs under the kernels of batch k + 1,
 * and the two batches' kernels never compete for the same CUs. */
int lfq_call_snvs_wait(lfq_ctx *ctx);
/* What the count kernel of this context's NEXT batch waits for on the device when the previous batch of the same GPU (any
 * context) is still running -- only matters to a caller that submits batch k + 1 before it waits for batch k:
 *   LFQ_GATE_TAIL  (default) that batch is past its row-bound DP kernels: the count kernel runs beside its folds, combines
 *                  and join (pays where the DP tail is long next to a short count kernel: 1000x);
 *   LFQ_GATE_END   all of that batch's kernels are done: batch after batch on the device with no host round trip between
 *                  them -- `submit(k + 1); wait(k); collect(k)` then hides every host latency without putting two batches'
 *                  kernels on the machine at once (the loop of lofreq_call.c:735-879 has no such gap to hide: it is serial);
 *   LFQ_GATE_NONE  nothing: it starts as soon as its stream is free.  The context then shapes its DP work for running BESIDE
 *                  a count kernel (a long column is cut into two row segments at most instead of eight: less work and
 *                  residency at the price of a longer chain, which is hidden there).
 * Results do not depend on the choice (p-values within the tolerance the parity tests hold every decomposition to).  LFQ_ERR_INVALID for another value. */
#define LFQ_GATE_TAIL 0
#define LFQ_GATE_END 1
#define LFQ_GATE_NONE 2
int lfq_set_batch_gate(lfq_ctx *ctx, int gate);
/* The stream this context's own launches go to (count kernels, BAQ, pileups; the DP chains always run on the device's three
 * shared DP streams).  By default every context of a GPU shares ONE: batches submitted through several contexts then run in
 * submission order, which is what a single thread that pipelines batches wants (and what the batch gates order).  A caller
 * that drives several contexts from several HOST THREADS (one region / bin per thread, as call-parallel's workers do) sets
 * on = 1 per context: the context gets a stream of its own, a thread's waits then cover its own work only and one thread's
 * BAQ kernels run beside another's pileups.  The batch gates do not apply to such a context.  Call it while the context is
 * idle (it synchronizes).  Results do not depend on the choice. */
int lfq_set_private_stream(lfq_ctx *ctx, int on);
/* h_counts_or_null: the dense entries, ncols of them.  Needs a batch whose dense entries are complete: LFQ_ERR_INVALID when
 * the batch was submitted after lfq_set_dense_counts(ctx, 0) (the entries of its untested columns were never written). */
int lfq_call_snvs_collect(lfq_ctx *ctx, lfq_conf *conf, lfq_snv_record *records, int64_t records_capacity,
                          int64_t *n_records, lfq_col_counts *h_counts_or_null, lfq_batch_stats *stats_out);

/* second half for a SHARDED run (N processes, below): the batch's sparse records as the device wrote them -- shard-local
 * running Bonferroni factors, no emit test yet.  The caller exchanges its test counts (lfq_shard_exchange_counts),
 * rebases the factors (lfq_shard_rebase_bonferroni) and then runs lfq_finalize_pvals.  conf is not advanced
 * (lfq_shard_advance_conf does that with the batch's stats->n_tested).  LFQ_ERR_CAPACITY: *n_pvals says how many. */
int lfq_call_snvs_collect_pvals(lfq_ctx *ctx, lfq_col_pvals *pvals, int64_t pvals_capacity, int64_t *n_pvals,
                                lfq_batch_stats *stats_out);

/* host finishing step of layer 2, exposed for tests: sparse device records -> reported SNVs */
int lfq_finalize_pvals(const lfq_conf *conf, const lfq_col_pvals *pvals, int64_t n_pvals,
                       const int32_t *coverage_plp_or_null, const uint8_t *ref_base,
                       lfq_snv_record *records, int64_t records_capacity, int64_t *n_records);
/* expl() + the reference's clamp; exposed for tests */
long double lfq_pvalue_from_log(double logp, int status);

/* --- layer 3: output and final filter --- */
int lfq_format_snv_record(char *buf, int buflen, const char *chrom, int64_t pos0,
                          const lfq_snv_record *rec, const char *filter_or_null);
/* all (kept) records of a batch; pos0_or_null == NULL uses rec.col as the 0-based position.
 * Returns the byte count of the full text (written only if it fits into buflen). */
int64_t lfq_format_vcf(char *buf, int64_t buflen, const char *chrom, const int64_t *pos0_or_null,
                       const lfq_snv_record *recs, int64_t n, const uint8_t *keep_or_null,
                       const char *filter_or_null);
int lfq_snvqual_thresh(float sig, int64_t bonf_subst);             /* lofreq_call.c:1523-1527 */
int lfq_sb_phred(int ref_fw, int ref_rv, int alt_fw, int alt_rv);  /* lofreq_call.c:117-129 */
double lfq_fisher_exact(int n11, int n12, int n21, int n22, double *left, double *right, double *two);
int64_t lfq_fdr(const double *pvals, int64_t n, double alpha, int64_t num_tests, int64_t *rejected_idx);
void lfq_bonf_corr(double *pvals, int64_t n, int64_t num_tests);
void lfq_holm_bonf_corr(double *pvals, int64_t n, double alpha, int64_t num_tests);
/* `lofreq filter` as `lofreq call` invokes it: keep[i] = 1 iff record i ends up PASS */
int lfq_filter_records(const lfq_snv_record *records, int64_t n, int snvqual_thresh,
                       int apply_defaults, uint8_t *keep);

/* --- `lofreq filter`, every mode (lofreq_filter.c:861-1331): what lfq_filter_records / lfq_filter_indel_records do for
 * the one configuration `lofreq call` passes, for any configuration of the command.  The reference works on the variants
 * of a VCF file in file order, SNVs and indels mixed; here a variant is the handful of fields the filters look at. */
typedef enum lfq_mtc_type {        /* mtc_type_t, multtest.h:33-39 */
    LFQ_MTC_NONE = 0,
    LFQ_MTC_BONF = 1,
    LFQ_MTC_HOLMBONF = 2,
    LFQ_MTC_FDR = 3
} lfq_mtc_type;

typedef struct lfq_filter_conf {    /* filter_conf_t, lofreq_filter.c:59-112 */
    int32_t only_snvs, only_indels;          /* --only-snvs / --only-indels: the other kind is dropped, not filtered */
    int32_t dp_min, dp_max;                  /* -v / -V; < 1 = off */
    float af_min, af_max;                    /* -a / -A; <= 0 = off */
    int32_t sb_thresh;                       /* -B: filter if SB > thresh (and the compound rule); 0 = off */
    int32_t sb_mtc_type;                     /* -b: lfq_mtc_type; conflicts with sb_thresh */
    double sb_alpha;                         /* -c */
    int64_t sb_ntests;                       /* 0 = the number of variants tested; set on return */
    int32_t sb_no_compound;                  /* --sb-no-compound: without "85 % of the alt bases on one strand" (:57, 214-236) */
    int32_t sb_incl_indels;                  /* --sb-incl-indels */
    int32_t snvqual_thresh;                  /* -Q: filter SNVs with -1 < QUAL < thresh; 0 = off */
    int32_t snvqual_mtc_type;                /* -q */
    double snvqual_alpha;                    /* -r */
    int64_t snvqual_ntests;                  /* -s; 0 = the number of SNVs; set on return */
    int32_t indelqual_thresh;                /* -K */
    int32_t indelqual_mtc_type;              /* -k */
    double indelqual_alpha;                  /* -l */
    int64_t indelqual_ntests;                /* -m */
} lfq_filter_conf;

/* main_filter's initial values (:1091-1097): everything off, the three alphas at DEFAULT_SIG 0.01 */
void lfq_filter_conf_init(lfq_filter_conf *conf);
/* what main_filter does after its options are parsed unless --no-defaults is given (:1184-1197): strand bias by FDR at
 * alpha 0.001 if neither -B nor -b was set, DP >= 10 if -v was not set.  Call it after setting the options. */
void lfq_filter_conf_defaults(lfq_filter_conf *conf);

typedef struct lfq_filter_var {     /* one variant as mtc_quals_from_vcf_file (:790-858) and the apply_* functions read it */
    int32_t is_indel;
    int32_t qual;                   /* QUAL; -1 = missing (counts as INT_MAX in the corrections, :824-831) */
    int32_t dp;                     /* INFO DP */
    int32_t sb;                     /* INFO SB (0 if absent, :845) */
    int32_t alt_fw, alt_rv;         /* DP4[2], DP4[3] */
    float af;                       /* INFO AF as strtof of its text (%f: six decimals) -- lfq_filter_var_from_* do that */
    int32_t pad_;
} lfq_filter_var;

/* bits of a variant's result */
#define LFQ_FILT_AF_MIN 1u
#define LFQ_FILT_AF_MAX 2u
#define LFQ_FILT_DP_MIN 4u
#define LFQ_FILT_DP_MAX 8u
#define LFQ_FILT_SNVQUAL 16u
#define LFQ_FILT_INDELQUAL 32u
#define LFQ_FILT_SB 64u
#define LFQ_FILT_DROPPED 128u       /* --only-snvs / --only-indels: not written at all */

/* fail[i] = the filters variant i fails, in the bit order the reference appends their ids to FILTER (:1255-1297);
 * 0 = PASS.  conf's *_ntests are filled in as the reference fills them in (:407-415).  Returns LFQ_ERR_INVALID for the
 * option conflicts main_filter rejects (:1205-1227). */
int lfq_filter_vars(lfq_filter_conf *conf, const lfq_filter_var *vars, int64_t n, uint32_t *fail);
/* the id one bit stands for (min_dp_10, sb_fdr, snvqual_bonf, min_snvqual_53, ...; cfg_filter_to_vcf_header,
 * :682-786); returns its length, 0 if that filter is off */
int lfq_filter_id(const lfq_filter_conf *conf, uint32_t bit, char *buf, int buflen);
/* the FILTER column of a variant: ids joined by ';' (vcf_var_add_to_filter, vcf.c:524-563), "PASS" for 0 */
int lfq_filter_string(const lfq_filter_conf *conf, uint32_t fail_bits, char *buf, int buflen);
/* the ##FILTER header lines the configuration adds, in the reference's order; returns the text's length */
int lfq_filter_header_lines(const lfq_filter_conf *conf, char *buf, int buflen);
void lfq_filter_var_from_snv(const lfq_snv_record *rec, lfq_filter_var *out);
void lfq_filter_var_from_indel(const lfq_indel_record *rec, lfq_filter_var *out);

/* --- `lofreq uniq --use-det-lim` (uniq_snv, lofreq_uniq.c:222-333): the second consumer of the
 * column boundary.  For every column (the pileup of the OTHER sample at a variant's position, built with uniq's
 * own mpileup settings: no BAQ, MAPQ >= 1, lofreq_uniq.c:461-465) and the variant's allele frequency af[col]:
 * would the variant have been detectable here?  The default varcall_conf (init_varcall_conf), the first alt count
 * replaced by (int)(af * n_err_probs) (float product, truncated), snpcaller(bonf 1, alpha 0.01f);
 * detectable[col] = pvalue * 1 < 0.01f, the condition under which uniq_snv adds the UNIQ flag.  Only the 'N'
 * reference gate applies (uniq_snv does not go through call_snvs).  pvalue_or_null[col] gets snpcaller's value for
 * the columns that were emitted (LDBL_MAX elsewhere: K = 0, or pruned as not significant).
 * An AF outside [0, 1] is reset like the reference does (af < 0 -> 0.01, af > 1 -> 1.0, lofreq_uniq.c:262-268), here
 * and in lfq_uniq_binom_batch; a NaN is LFQ_ERR_INVALID. */
int lfq_uniq_detlim_batch(lfq_ctx *ctx, const lfq_tracks *tracks, int tracks_on_device, const float *af,
                          uint8_t *detectable, long double *pvalue_or_null);

/* --- `lofreq uniq`, default mode (uniq_snv's binomial branch, lofreq_uniq.c:335-393, + apply_uniq_filter_mtc, :140-206).
 * Per column (the other sample's pileup at a variant's position, uniq's own mpileup settings as above): coverage =
 * coverage_plp (tracks->coverage_plp, or the observation count), alt_count = the bases of nucleotide alt_base[col] in
 * the column whatever their quality (base_count, plp.c:128-132; counted on the device), pvalue =
 * binom(coverage, alt_count, af) = P(X <= alt_count), X ~ Binomial(coverage, af) (binom.c:52-69 -> cdflib90's cdfbin),
 * uq_out[col] = PROB_TO_PHREDQUAL_SAFE(pvalue), the value of the UQ= INFO tag; -1 where the reference adds none
 * (coverage < 1, or cdfbin rejects its arguments).  SNVs only (indel variants take their count from the event table,
 * which is host data: lfq_indel_columns; lfq_readset_uniq below counts them on the device).  lfq_uniq_mtc then decides PASS / uq_<mtc> like apply_uniq_filter_mtc:
 * mtc_type 1 bonf, 2 holm, 3 fdr (multtest.h; `lofreq uniq` defaults: fdr, alpha 0.001, ntests 0 = the number of
 * variants).  lfq_binom_cdf is the scalar test itself (status: cdfbin's code, 0 = ok). */
int lfq_uniq_binom_batch(lfq_ctx *ctx, const lfq_tracks *tracks, int tracks_on_device, const float *af,
                         const char *alt_base, int32_t *uq_out, double *pvalue_or_null);
int lfq_uniq_mtc(const int32_t *uq, int64_t n, int mtc_type, double alpha, int64_t ntests, uint8_t *pass);
double lfq_binom_cdf(int n, int k, double pr, int *status_or_null);

/* --- `lofreq uniq` on the reads of a resident read set (the read-level road to the two tests above) ----------------------
 * The reference runs one index query and one 1-bp mpileup per variant (lofreq_uniq.c:695-728).  Here: the reads of the
 * variants' span in ONE read set (the other sample's, filtered by the caller as uniq's mpileup filters them: MAPQ >= 1, no
 * orphans unless --use-orphan, the flag mask; no BAQ), and one sparse pileup for all variants.
 *
 * lfq_readset_pileup_sites: the pileup of a resident read set at a LIST of reference positions: column i = site i, in the order
 * given (any order, duplicates allowed); a site no read covers is an EMPTY column (mpileup would not call back at all).
 * tracks_out gets device tracks with ncols = n_sites: nt one byte per observation (LFQ_TRACKS_NT_PACKED is never set: the
 * columns are few and scattered, and both uniq entry points read unpacked tracks), the observations of a column in pileup
 * (read) order with the bytes lfq_readset_pileup_snv writes, ref_base from the contig, coverage_plp / num_bases as that function
 * sets them, baq always there (255 = missing where the read set has no BAQ), sq when the read set has source qualities.
 * coverage_plp_out_or_null / num_tails_out_or_null: [n_sites] host arrays; num_tails counts the entries that are the last
 * aligned base of their read (plp.c:912-920).  The buffers are the context's own, grow only, and are valid until the next
 * lfq_readset_pileup_sites or lfq_readset_uniq call on the context; they are NOT those of the region pileup:
 * lfq_pileup_skip_snv_columns and tracks returned earlier by lfq_readset_pileup_snv are untouched.  The call returns when the
 * tracks are complete.  Two kernels whatever the number of sites; per site 16 bytes come back between them and 21 go down.
 * LFQ_ERR_INVALID, before anything is launched: a NULL ctx, rs or tracks_out (before a device is touched); n_sites < 0; NULL
 * site_pos with n_sites > 0; a position outside [0, ref_len); reads that are not position-sorted (lfq_set_pileup_unsorted does
 * not apply); a context cap (lfq_set_max_depth) under which lfq_readset_kept_reads drops at least one read -- the reference
 * applies -d to the reads of each 1-bp query, not to the region's, and that rule is not approximated.  n_sites = 0: LFQ_OK, no
 * launch, ncols = 0. */
int lfq_readset_pileup_sites(lfq_ctx *ctx, lfq_readset *rs, const int64_t *site_pos, int64_t n_sites, int min_plp_bq,
                             lfq_tracks *tracks_out, int32_t *coverage_plp_out_or_null, int32_t *num_tails_out_or_null);

/* lfq_readset_uniq: uniq_snv (lofreq_uniq.c:222-394) for all variants at once, SNVs and indels, both modes.
 *   is_indel = strlen(REF) > 1 || strlen(ALT) > 1 || the INDEL key (vcf.c:328-337).
 *   coverage = coverage_plp, minus num_tails for an indel variant (:248-251); coverage < 1: no tag, no flag (:252-254), in BOTH
 *      modes -- with --use-det-lim an indel variant whose reads all end at the site has a non-empty column and detectable = 0.
 *   Default mode (use_det_lim = 0): alt_count = base_count of ALT[0] for an SNV (the nucleotide-count kernel of
 *      lfq_uniq_binom_batch), for an indel variant the number of pileup entries whose indel is the variant's (:343-368): the
 *      entry's position is the last of its M / = / X / D / N operation and an I or D follows (a P in between as htslib's
 *      resolve_cigar2 takes it), whatever the base's quality and BI / BD (uniq's min_plp_idq is 0, :460); an insertion's key is
 *      the inserted read letters (an ambiguity code is its own letter), a deletion's the contig letters pos + 1 .. pos + len
 *      upper-cased, 'N' beyond ref_len (plp.c:1091-1094, 1135-1138); a match is bytewise equality with REF + 1 if strlen(REF) >
 *      strlen(ALT), else ALT + 1; an empty key matches nothing.  Then pvalue = lfq_binom_cdf(coverage, alt_count, af) with the
 *      AF reset of :262-268, and uq = PROB_TO_PHREDQUAL_SAFE(pvalue); uq = -1 and pvalue = -1.0 where the reference adds no tag.
 *      detectable = 0.
 *   --use-det-lim (use_det_lim != 0): lfq_uniq_detlim_batch on the device tracks; alt_count = 0, uq = -1, pvalue = -1.0.
 *   Deletion keys and the reference's binary: `lofreq uniq` opens no FASTA, so its mpileup has no contig and the key of EVERY
 *      deletion is 'N' repeated there (plp.c:1136); here the key comes from the read set's contig.  The two agree where the
 *      contig holds N (or is all N, which the default mode reads for nothing else); INTEGRATION.md section 8.
 * One sparse pileup (lfq_readset_pileup_sites with the variants' keys, the event match done in its count pass); no
 * per-observation byte crosses the link in either direction.  The read-level filters are the caller's, as for every read set.
 * LFQ_ERR_INVALID, before anything is launched: a NULL ctx, rs, vars or out (before a device is touched); n < 0; a NULL array of
 * vars with n > 0 (indel_key_or_null excepted); offsets that decrease; a NaN in af; and everything lfq_readset_pileup_sites
 * refuses.  n = 0: LFQ_OK, no launch.  More than one contig per call and the per-query -d rule are not covered; the variants of a VCF
 * text: lfq_vcf_uniq_variants. */
typedef struct lfq_uniq_variants {
    int64_t n;
    const int64_t *pos;               /* [n] var->pos, 0-based */
    const int64_t *ref_off, *alt_off; /* [n + 1] into ref / alt */
    const char *ref, *alt;            /* REF / ALT strings, concatenated, no NULs */
    const uint8_t *indel_key_or_null; /* [n] vcf_var_has_info_key(var, "INDEL"); NULL = none has it */
    const float *af;                  /* [n] strtof of AF, or --uni-freq */
} lfq_uniq_variants;
typedef struct lfq_uniq_result {      /* caller's arrays, [n] each, any may be NULL */
    int32_t *coverage;    /* coverage_plp, minus num_tails for an indel variant (lofreq_uniq.c:248-251); 0 = uncovered */
    int32_t *alt_count;   /* default mode: base_count of ALT[0], or the event count of an indel variant */
    int32_t *uq;          /* default mode: the UQ= value; -1 where the reference adds no tag */
    double *pvalue;       /* default mode: binom()'s value, -1.0 where none */
    uint8_t *detectable;  /* --use-det-lim: 1 where the reference adds UNIQ */
} lfq_uniq_result;
int lfq_readset_uniq(lfq_ctx *ctx, lfq_readset *rs, const lfq_uniq_variants *vars, int use_det_lim, int min_plp_bq,
                     lfq_uniq_result *out);
/* the two kernels of the context's last lfq_readset_pileup_sites / lfq_readset_uniq call on the device's clock, the call's sites
 * and the observations of its columns; n_launches = 0 (and 0 ms) where nothing was launched */
typedef struct lfq_sites_times {
    double count_ms, scatter_ms;
    int64_t n_sites, n_obs;
    int n_launches;
} lfq_sites_times;
int lfq_last_sites_times(lfq_ctx *ctx, lfq_sites_times *t);

/* --- `lofreq plpsummary` / --plp-summary-only: the header line of plp_summary on a read set (lofreq_call.c:438-459) ---------
 * lfq_readset_plp_summary: for every covered position of [region_begin, region_end), in order and numbered as the columns of
 * lfq_readset_pileup_snv / lfq_readset_pileup_indels, what plp_summary prints in its first line:
 *   fw / rv      fw_counts / rv_counts in A, C, G, T, N order: the entries that are not deleted / skipped and have
 *                bq >= min_plp_bq, by seq_nt16_int code (every code above 4 is N) and strand (plp.c:929-941, 1007-1011);
 *   num_heads / num_tails   entries at the first / last aligned position of their read that are not deleted / skipped, BEFORE
 *                the min_plp_bq filter (plp.c:912-920); num_tails equals lfq_indel_columns.num_tails;
 *   the consensus (plp.c:1231-1268): cons_kind 0 = a base, cons_nt = bam_nt4_rev_table[argmax_d(base_counts)] with
 *                base_counts[nt4] += 1.0 - pow(10, -bq / 10.0), bq capped at 93 (:949-953), an increment of 0.0 replaced by
 *                DBL_MIN (:1003-1005), summed in pileup order, the first maximum winning (utils.c:87-98: N never wins a tie, a
 *                column without a kept base gets 'A'); cons_kind 1 / 2 = an insertion / deletion: per side the FIRST event in table
 *                order whose cons_quals (the sum of its reads' indel qualities) is strictly greatest, if that sum is strictly
 *                greater than the side's non-event quality sum; an insertion before a deletion.  Its key is
 *                cons_key_chars[cons_key_off[col] .. cons_key_off[col + 1]) (empty for kind 0; cons_nt is filled in either way).
 *                cons_kind != 0 exactly where lfq_indel_columns.cons_indel is set;
 *   num_ins / num_dels / hrun / coverage_plp / ref_base   those of lfq_readset_pileup_indels for the same region and
 *                min_plp_idq, which this call RUNS: afterwards the context's current lfq_indel_columns are this region's, exactly
 *                as after lfq_readset_pileup_indels (an IndelColumns obtained earlier is superseded).
 * One kernel, one wavefront per column; a double sum depends on the order of its terms, so a column whose two largest sums are
 * closer than the rounding of two summation orders can explain is summed again in pileup order, add by add (lfq_summary_times.
 * n_ordered counts them).  A -d cap (lfq_set_max_depth) removes reads as in the other pileups.  The arrays are host memory owned
 * by the context, grow only, valid until the next lfq_readset_plp_summary call on it; the SNV tracks of lfq_readset_pileup_snv
 * and the buffers of lfq_readset_pileup_sites are untouched.
 * LFQ_ERR_INVALID, before anything is launched: a NULL ctx, rs or out (before a device is touched); region_end < region_begin; a
 * region outside [0, ref_len]; min_plp_bq < 0; reads that are not position-sorted (lfq_set_pileup_unsorted does not apply).  An
 * empty region, an empty read set or a region no read covers: LFQ_OK, ncols = 0, no summary launch.
 * The indented quality lines of plp_summary (lofreq_call.c:460-598) come from lfq_plp_quals_from_tracks + lfq_format_plp_quals (the
 * nucleotide lines) and lfq_format_plp_indel_quals (the indel lines and the closing empty line), below. */
typedef struct lfq_plp_summary {
    int64_t ncols;
    const int64_t *col_pos;            /* [ncols] 0-based positions */
    const uint8_t *ref_base;           /* [ncols] plp.c:818-823 */
    const int32_t *fw, *rv;            /* [ncols][5] A, C, G, T, N */
    const int32_t *num_heads, *num_tails, *num_ins, *num_dels, *hrun, *coverage_plp;   /* [ncols] */
    const uint8_t *cons_kind;          /* [ncols] 0 base, 1 '+', 2 '-' */
    const uint8_t *cons_nt;            /* [ncols] 'A' 'C' 'G' 'T' 'N' */
    const int64_t *cons_key_off;       /* [ncols + 1] */
    const char *cons_key_chars;
} lfq_plp_summary;
int lfq_readset_plp_summary(lfq_ctx *ctx, lfq_readset *rs, int64_t region_begin, int64_t region_end, int min_plp_bq,
                            int min_plp_idq, const lfq_plp_summary **out);
/* "chrom\tpos\tref\tcons\tA:fw/rv\tC:..\tG:..\tT:..\tN:..\theads:%d\ttails:%d\tins:%d\tdels:%d\thrun:%d\n" of column col
 * (lofreq_call.c:445-459).  Returns the length of the line (without the NUL) when buflen holds line and NUL, else
 * LFQ_ERR_CAPACITY; LFQ_ERR_INVALID for a NULL argument or a column outside [0, ncols). */
int lfq_format_plp_summary(char *buf, int buflen, const char *chrom, const lfq_plp_summary *summary, int64_t col);
/* the kernel of the context's last lfq_readset_plp_summary call on the device's clock, its columns and how many of them took
 * the ordered path; n_launches = 0 (and 0 ms) where nothing was launched */
typedef struct lfq_summary_times {
    double kernel_ms;
    int64_t n_cols, n_ordered;
    int n_launches;
} lfq_summary_times;
int lfq_last_summary_times(lfq_ctx *ctx, lfq_summary_times *t);

/* --- the quality lines of plp_summary (lofreq_call.c:460-598) ---------------------------------------------------------------
 * lfq_plp_quals_from_tracks: the bq / baq / mq / sq bytes of the columns [col_begin, col_end) of SNV tracks, per column stably
 * partitioned by nucleotide code in A, C, G, T, N order (a code above 4 counts as N) -- base_quals[nt4], baq_quals[nt4],
 * map_quals[nt4], source_quals[nt4] of plp_col_t (plp.c:954-975) -- with pileup order kept inside each group, and the five
 * group sizes of every column as offsets.  One kernel (lfq_plp_group_kernel), one wavefront per column.
 * tracks_on_device != 0: the tracks lfq_readset_pileup_snv / lfq_pileup_snv_tracks / lfq_readset_pileup_sites returned; the
 * kernel is queued behind their scatter pass on the context's stream.  Otherwise host tracks, whose columns of the range are
 * uploaded into the context's buffers.  The column range lets a caller page through a region: the output is as large as the
 * tracks of the range.  The results are pinned host memory owned by the context, grow only, valid until the next call of this
 * function on it; the SNV tracks, the buffers of lfq_readset_pileup_sites and the arrays of lfq_readset_plp_summary are
 * untouched.
 * Observations are in the reference's order only where the tracks are: that holds for position-sorted reads (the column-major
 * kernels), and is NOT promised for tracks made under lfq_set_pileup_unsorted.
 * LFQ_ERR_INVALID, before anything is launched: a NULL ctx, tracks or out (before a device is touched); a range outside
 * [0, tracks->ncols] or col_end < col_begin; LFQ_TRACKS_NT_PACKED tracks (lfq_set_pileup_nt_packed(ctx, 0) gives byte tracks).
 * An empty range or a range without observations: LFQ_OK, no launch (lfq_plp_quals_times.n_launches = 0). */
typedef struct lfq_plp_quals {
    int64_t ncols, col_begin;          /* columns [col_begin, col_begin + ncols) of the tracks */
    const int64_t *nt_off;             /* [5 * ncols + 1]: group (column i, nt k) = [nt_off[5i + k], nt_off[5i + k + 1]) */
    const uint8_t *bq, *baq, *mq, *sq; /* grouped bytes, track encoding unchanged; baq / sq NULL when the tracks have none */
} lfq_plp_quals;
int lfq_plp_quals_from_tracks(lfq_ctx *ctx, const lfq_tracks *tracks, int tracks_on_device,
                              int64_t col_begin, int64_t col_end, const lfq_plp_quals **out);
/* lofreq_call.c:460-489 for column col (a column index of the TRACKS, inside the struct's range): for every nucleotide with a
 * non-empty group, in A C G T N order, the lines "  %c\tBQ =\t", BAQ, MQ and, with LFQ_USE_SQ in flag, SQ, each followed by
 * " %d" per value and "\n".  BQ: the byte.  BAQ: -1 for every value unless LFQ_USE_BAQ is in flag (:478), else the byte with
 * 255 -> -1.  MQ: the byte as it is (255 prints 255).  SQ: 255 -> -1, 254 -> 49314 (the one value above 253 source_qual returns,
 * plp.c:521).  LFQ_USE_BAQ without a baq array or LFQ_USE_SQ without an sq array: LFQ_ERR_INVALID (the reference would read an
 * empty array).  Returns the length written (without the NUL); buf == NULL && buflen == 0: the length needed (lines grow with
 * the depth); LFQ_ERR_CAPACITY when text and NUL do not fit; LFQ_ERR_INVALID for a NULL struct or a column outside its range.
 * Pure host code. */
int lfq_format_plp_quals(char *buf, int64_t buflen, const lfq_plp_quals *q, int64_t col, int flag);
/* on = 1: from then on lfq_readset_pileup_indels / lfq_pileup_indel_columns (and the indel pileup lfq_readset_plp_summary runs)
 * give ne_off / ne_q / ne_mq -- ins_quals / ins_map_quals, del_quals / del_map_quals -- for EVERY column, not only for those
 * with an event: what plp_summary's "+0" / "-0" lines print.  Costs 8 bytes per observation and region (two int16 per side) on
 * the device and, with lfq_set_indel_arrays_on_host(ctx, 1) -- which lfq_format_plp_indel_quals needs --, in the copy back.
 * lfq_call_indels_batch reads the arrays at event columns only (through ne_off): same records.  Default 0: every byte as before. */
int lfq_set_indel_arrays_all_columns(lfq_ctx *ctx, int on);
/* lofreq_call.c:491-598 for column col: "  +0\tIDQ =\t" / "  +0\tMQ =\t" over the reads without an insertion, every insertion
 * event in table order ("  +KEY\tIQ =\t", MQ, AQ, SQ), the same for "-0" and the deletion events (IDQ, MQ, AQ, SQ), and the
 * closing empty line.  Values are the int16 entries as they are (-1 = missing); rd_sq saturates at 32767, which prints as 49314.
 * Return rules of lfq_format_plp_quals.  LFQ_ERR_INVALID also when ne_q / ne_mq are NULL (device-only arrays), or when the column
 * has non-event reads by its counts but an empty ne_off range (lfq_set_indel_arrays_all_columns off). */
int lfq_format_plp_indel_quals(char *buf, int64_t buflen, const lfq_indel_columns *cols, int64_t col);
/* the kernel of the context's last lfq_plp_quals_from_tracks call on the device's clock, its columns and observations;
 * n_launches = 0 (and 0 ms) where nothing was launched */
typedef struct lfq_plp_quals_times { double kernel_ms; int64_t n_cols, n_obs; int n_launches; } lfq_plp_quals_times;
int lfq_last_plp_quals_times(lfq_ctx *ctx, lfq_plp_quals_times *t);

/* --- synthetic workload (bench / tests): fills device tracks per include/lofreq_synth.h --- */
int lfq_synth_fill_device(lfq_ctx *ctx, uint64_t seed, uint32_t depth, uint32_t plant_period,
                          int64_t col_begin, int64_t ncols, uint8_t *d_nt, uint8_t *d_bq,
                          uint8_t *d_baq, uint8_t *d_mq, uint64_t *d_col_off, uint8_t *d_ref_base,
                          void *stream);
/* same, with the nt track in the LFQ_TRACKS_NT_PACKED layout if nt_packed != 0 (d_nt then needs half the bytes) */
int lfq_synth_fill_device_layout(lfq_ctx *ctx, uint64_t seed, uint32_t depth, uint32_t plant_period,
                                 int64_t col_begin, int64_t ncols, uint8_t *d_nt, uint8_t *d_bq,
                                 uint8_t *d_baq, uint8_t *d_mq, uint64_t *d_col_off, uint8_t *d_ref_base,
                                 int nt_packed, void *stream);

/* --- device timing of the last batch (HIP events on the stream the kernels ran on) --- */
typedef struct lfq_kernel_times {
    float ms_count;     /* sum over the batch's segments of the count kernel launches */
    float ms_scan;      /* sum of the scan (prefix + work-list) kernels */
    float ms_dp;        /* DP time not hidden under a count kernel: last count kernel end -> all done */
    float ms_total;     /* first kernel start -> all done */
    float ms_dp_light, ms_dp_mid, ms_dp_big;    /* sums of the concurrent DP kernels' own durations */
    int32_t n_segments; /* count-kernel launches in this batch */
} lfq_kernel_times;
int lfq_last_kernel_times(lfq_ctx *ctx, lfq_kernel_times *t);
/* the BAQ kernels of the context's last lfq_readset_baq call (waits for them): first narrow-band launch -> everything done,
 * on the device's clock; the main-stream launches in between; the call's reads and bases.  All 0 before the first call. */
typedef struct lfq_baq_times {
    float ms_kernels;
    int32_t n_launches;
    int64_t n_reads, n_bases;
} lfq_baq_times;
int lfq_last_baq_times(lfq_ctx *ctx, lfq_baq_times *t);

/* --- DP work of the last batch (device counters; SURVEY 8d "ALGORITHMIC DP work", the secondary roofline) ---
 * cells = sum over the tested columns of sum_{n = 1..N*} min(n, K): N* = the kept row at which this implementation's
 * pruning test fired (track order; the reference sorts its probabilities ascending and therefore prunes LATER, so
 * its own cell count for the same columns is larger), or the column's end.  Columns finished by the underflow
 * shortcut count only the rows their remaining recurrence ran.  A light column that the screen kernel hands to the
 * retry kernel is counted in both (the work was done twice). */
typedef struct lfq_dp_work {
    int64_t cells;             /* recurrence cells processed */
    int64_t rows;              /* kept rows processed */
    int64_t n_light, n_mid, n_big;   /* tested columns per scheduling class */
    int64_t n_light_retry;     /* light columns finished by the one-column-per-wavefront kernel */
    int64_t bytes_read_count;  /* track + header bytes the count kernel instantiation of this batch reads (layout bytes) */
    int64_t bytes_written_count; /* dense records (of the tested columns only where lfq_set_dense_counts(0) applies) + class flags it writes */
    int64_t n_approx_pruned;   /* tested columns the Poisson gate (lfq_conf.approx_threshold_n) gave up: not in the classes above */
} lfq_dp_work;
int lfq_last_dp_work(lfq_ctx *ctx, lfq_dp_work *w);

/* --- N processes, one per GPU: the exchange of a sharded run, from C ---
 * The reference's `call-parallel` wrapper runs one `lofreq call -r <bin>` per worker and merges afterwards: it sums the
 * per-worker test counts it parses from the logs and concatenates the VCFs (lofreq2_call_pparallel.py:131-185, 685-707).
 * Here every process calls its shard with the SAME starting conf (layer 1 or 2), then:
 *     lfq_shard_exchange_counts   one all-gather of a few int64 per rank (tested columns, indel tests) -> every rank's
 *                                 counts and this rank's exclusive prefix
 *     lfq_shard_rebase_bonferroni the shard-local running Bonferroni factors of the sparse p-value records become the
 *                                 single-process ones (3 tests per tested column of the earlier shards,
 *                                 lofreq_call.c:794-801); lfq_finalize_pvals then applies the exact emit test
 *     lfq_shard_gather_records    every rank's reported variants, in shard order, `col` made global by col_offset;
 *                                 every rank takes part whatever its `capacity` (0 on the ranks that do not want the
 *                                 records): too little room returns LFQ_ERR_CAPACITY with *n_out = the total
 *     lfq_shard_advance_conf      conf->bonf_subst / num_snv_tests as after the single-process loop over all shards
 * `comm` is an ncclComm_t of RCCL (one rank per process, created by the caller: ncclCommInitRank) or NULL when
 * world == 1.  RCCL is looked up at run time (dlopen of librccl): the library has no link-time dependency on it.
 * lofreq_amd/shard.py calls these same functions (round 6: ONE implementation of the exchange; torch.distributed only
 * carries the ncclUniqueId to the ranks and, as a gloo group, serves as the host transport for the counts). */
/* A launcher that has no RCCL communicator (MPI, a shared directory, a test double) supplies the one collective the
 * exchange needs: all-gather of `bytes` bytes per rank, host buffers, recv = world * bytes in rank order; 0 = ok.
 * While set (process-wide; NULL restores RCCL) `comm` is ignored by the lfq_shard_* calls. */
typedef int (*lfq_host_allgather_fn)(void *user, int world, int rank, const void *send, void *recv, size_t bytes);
int lfq_shard_set_host_allgather(lfq_host_allgather_fn fn, void *user);
/* The library's own host transport for the ranks of ONE node: an all-gather through a POSIX shared-memory segment (a slot
 * per rank, double-buffered, sequence numbers with release / acquire order; microseconds where a loopback TCP ring takes
 * milliseconds at eight ranks).  lfq_shard_shm_open maps /dev/shm<name> (created by whoever comes first; `name` = "/..." and
 * NEW PER RUN -- a nonce every rank of the run knows) and installs it as the host all-gather; once every rank has opened
 * it (any barrier, e.g. a first all-gather through it), one rank calls lfq_shard_shm_unlink so that nothing is left behind
 * if the run dies; lfq_shard_shm_close unmaps and uninstalls. */
int lfq_shard_shm_open(const char *name, int world, int rank);
int lfq_shard_shm_unlink(void);
int lfq_shard_shm_close(void);
/* the collective itself: `bytes` bytes of every rank, in rank order (all = world * bytes) */
int lfq_shard_allgather(lfq_ctx *ctx, void *comm, int world, int rank, const void *mine, int64_t bytes, void *all);
int lfq_shard_exchange_counts(lfq_ctx *ctx, void *comm, int world, int rank, const int64_t *local, int n,
                              int64_t *all_out /* [world][n] */, int64_t *prefix_out /* [n] */);
int lfq_shard_rebase_bonferroni(lfq_col_pvals *pvals, int64_t n, int64_t prefix_tested);
int lfq_shard_gather_records(lfq_ctx *ctx, void *comm, int world, int rank, const lfq_snv_record *recs, int64_t n,
                             int64_t col_offset, lfq_snv_record *out, int64_t capacity, int64_t *n_out);
int lfq_shard_advance_conf(lfq_conf *conf, int64_t total_tested);
/* The gather in two halves, for a caller that pipelines steps (bench.py's sharded step, lofreq_amd/shard.py): every rank hands
 * over ONE piece of `piece_bytes` bytes (the same size on every rank; what is inside -- a record count in front of a fixed
 * number of record slots -- is the caller's business).  _start returns at once: with a communicator the piece goes up from
 * a pinned copy, the collective (ncclAllGather) and -- where want_all is set -- the copy of all pieces back to pinned memory
 * are queued on a high-priority stream of the handle's own, and nothing waits for the device; without one (a host transport
 * set by lfq_shard_set_host_allgather, or world == 1) the blocking all-gather runs inside _start.  _wait blocks until this
 * rank's side is done and copies the world * piece_bytes bytes in rank order into `all` (NULL, or a rank that did not set
 * want_all: nothing is copied).  Unlike the blocking calls above, _start uses the communicator when one is given even
 * while a host transport is set: the test counts are host integers and take the host road, the records the device's.
 * Every rank must call _start and _wait for every gather, in the same order. */
typedef struct lfq_shard_gather lfq_shard_gather;
int lfq_shard_gather_start(lfq_ctx *ctx, void *comm, int world, int rank, const void *piece, int64_t piece_bytes,
                           int want_all, lfq_shard_gather **handle_out);
int lfq_shard_gather_wait(lfq_shard_gather *handle, void *all_or_null, int64_t all_bytes);

#ifdef __cplusplus
}
#endif
#endif
