/*
 * lfq_ctx.h -- what the host-side files of the library share: the context (lfq_ctx), the helper-thread pool of the
 * host loops, grow-only device buffers, the pinned pool, and the few internal functions that cross file boundaries.
 * Internal: nothing outside lofreq_amd/csrc includes it.
 *
 *   lfq_api.hip        context, streams, the batch driver (layer 1), the call_snvs loop (layer 2), uniq, generator
 *   lfq_indel_api.hip  the indel tests (lfq_call_indel_tests_batch, lfq_call_indels_batch)
 *   lfq_readset.hip    the resident read set: upload, BAQ / IDAQ, source quality, both pileups
 *   lfq_plp_indel_host.h   the host stages of its indel pileup, plain C++ (and the columns it hands out, LfqIndelColsOwned)
 *   lfq_bamrec.hip     BAM records decoded and rewritten on the device: kernels and their launches (for lfq_readset.hip)
 *   lfq_bgzf.hip       BGZF blocks inflated on the device (over lfq_inflate.h), the record scan, lfq_readset_create_from_bgzf
 *   lfq_bgzf_deflate.hip   bytes cut into BGZF blocks and compressed on the device (over lfq_deflate.h)
 *   lfq_bamidx.hip         the .bai of a BAM from its records and block tables (over lfq_bamidx.h)
 *   lfq_bed.hip            the targets of `lofreq call -l`: the BED itself, lfq_set_bed, the read and column kernels (over lfq_bed.h)
 *   lfq_fasta.hip          `lofreq faidx` and the contig of a FASTA: scan, line and entry kernels, both fetch paths (over lfq_fasta.h)
 *   lfq_vcf.hip            VCF text parsed on the device and `lofreq vcfset`: scan, parse, runs, match, plan / copy (over lfq_vcf.h)
 *   lfq_tbx.hip            the .tbi of a bgzipped VCF from an open file's table, and a region opened through one (over lfq_tbx.h)
 *   lfq_shard.hip      device choice of a worker, the exchange of a sharded run
 */
#ifndef LFQ_CTX_H
#define LFQ_CTX_H

#include <hip/hip_runtime.h>

#include <ctype.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <atomic>
#include <functional>
#include <unistd.h>
#include <fcntl.h>
#include <sys/file.h>
#include <thread>
#include <vector>

#include "lfq_internal.h"
#include "lfq_plp_indel_host.h"
#include "lfq_bed.h"
#include "lofreq_synth.h"

#define LFQ_TRY_HIP(expr)           \
    do {                            \
        hipError_t e_ = (expr);     \
        if (e_ != hipSuccess) {     \
            return LFQ_ERR_HIP;     \
        }                           \
    } while (0)

#define LFQ_TRY(expr)               \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != LFQ_OK) {        \
            return rc_;             \
        }                           \
    } while (0)

static inline double lfq_now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define lfq_timing_on (lfq_knobs().timing != 0)

/* The helper threads of the host loops below.  A region's steps run a dozen such loops milliseconds apart; threads
 * created (or woken from a condition variable) per loop start on idle cores and the same loop took anything between
 * 0.7 and 4.5 ms (BAQ geometry of 400 K reads, 4 threads; one thread: 2.4 ms).  These seven stay: after a loop they spin
 * for LFQ_HOST_SPIN_US (2000) microseconds waiting for the next one before they go to sleep.  One loop at a time
 * (try_run fails when another thread is using the pool, and in a forked child: the caller then creates threads). */
#if defined(__x86_64__) || defined(__i386__)
#define LFQ_CPU_PAUSE() __builtin_ia32_pause()
#elif defined(__aarch64__)
#define LFQ_CPU_PAUSE() __asm__ __volatile__("yield")
#else
#define LFQ_CPU_PAUSE() std::this_thread::yield()
#endif

/* most threads a host loop is cut for (the arrays of per-part results are this long); how many it really uses:
 * LFQ_HOST_LOOP_THREADS, the process's CPU budget, the loop's length */
#define LFQ_HOST_PARTS 16

class LfqLoopPool {
public:
    static LfqLoopPool &instance()
    {
        static LfqLoopPool p;
        return p;
    }
    bool try_run(int parts, const std::function<void(int)> &task)       /* task(1 .. parts - 1) here, part 0 by the caller */
    {
        if (parts - 1 > (int)th_.size() || getpid() != pid_ || !call_m_.try_lock()) {
            return false;
        }
        /* every helper acknowledges every generation (those beyond `parts` without running anything): none of them can
         * still be looking at this generation's task when the next one is written */
        job_ = &task;
        want_ = parts - 1;
        pending_.store((int)th_.size(), std::memory_order_relaxed);
        /* W gen_ then R sleepers_ here, W sleepers_ then R gen_ in the helper: sequentially consistent on both sides,
         * so that at least one of them sees the other's write and no wake-up is lost on a weaker memory model */
        gen_.fetch_add(1, std::memory_order_seq_cst);
        if (sleepers_.load(std::memory_order_seq_cst) > 0) {
            { std::lock_guard<std::mutex> lk(m_); }
            cv_.notify_all();
        }
        return true;
    }
    void finish()                                                        /* after the caller's own part */
    {
        while (pending_.load(std::memory_order_acquire) > 0) {
            LFQ_CPU_PAUSE();
        }
        job_ = nullptr;
        call_m_.unlock();
    }

private:
    LfqLoopPool() : pid_(getpid())
    {
        spin_us_ = lfq_knobs().host_spin_us;
        /* the helpers spin between loops: a node's ranks share its cores (LOCAL_WORLD_SIZE processes) */
        const unsigned hw = std::max(1u, lfq_cpu_budget() / (unsigned)std::max(lfq_knobs().local_world_size, 1));
        const unsigned want = (unsigned)std::min<long>(std::max<long>(lfq_knobs().host_loop_threads, 1), LFQ_HOST_PARTS);
        const int n = spin_us_ < 0 ? 0 : (int)std::min(want - 1u, hw - 1u);
        for (int i = 0; i < n; i++) {
            th_.emplace_back([this, i] { loop(i); });
        }
    }
    ~LfqLoopPool()
    {
        if (getpid() != pid_) {                 /* a forked child: the threads stayed with the parent */
            for (auto &t : th_) {
                t.detach();
            }
            return;
        }
        stop_.store(true);
        gen_.fetch_add(1, std::memory_order_seq_cst);
        { std::lock_guard<std::mutex> lk(m_); }
        cv_.notify_all();
        for (auto &t : th_) {
            t.join();
        }
    }
    void loop(int idx)
    {
        uint64_t seen = 0;
        for (;;) {
            const double t0 = lfq_now_ms();
            int polls = 0;
            while (gen_.load(std::memory_order_acquire) == seen) {
                LFQ_CPU_PAUSE();
                if ((++polls & 255) == 0 && (lfq_now_ms() - t0) * 1e3 > (double)spin_us_) {
                    std::unique_lock<std::mutex> lk(m_);
                    sleepers_.fetch_add(1, std::memory_order_seq_cst);
                    cv_.wait(lk, [&] { return gen_.load(std::memory_order_seq_cst) != seen; });
                    sleepers_.fetch_sub(1, std::memory_order_seq_cst);
                }
            }
            if (stop_.load()) {
                return;
            }
            seen = gen_.load(std::memory_order_acquire);
            if (idx < want_ && job_) {
                (*job_)(idx + 1);
            }
            pending_.fetch_sub(1, std::memory_order_release);
        }
    }
    std::vector<std::thread> th_;
    std::mutex call_m_, m_;
    std::condition_variable cv_;
    std::atomic<uint64_t> gen_{0};
    std::atomic<int> pending_{0}, sleepers_{0};
    std::atomic<bool> stop_{false};
    const std::function<void(int)> *job_ = nullptr;
    int want_ = 0;
    long spin_us_ = 2000;
    pid_t pid_;
};

/* f(part) for part in [0, n_parts), part 0 here: the others on the pool's helpers when it is free, else on threads of their own */
template <typename F>
static void lfq_run_parts(int n_parts, F f)
{
    const std::function<void(int)> task = [&](int p) { f(p); };
    if (n_parts > 1 && LfqLoopPool::instance().try_run(n_parts, task)) {    /* (one part: the pool is not even created) */
        f(0);
        LfqLoopPool::instance().finish();
        return;
    }
    std::vector<std::thread> th;
    for (int p = 1; p < n_parts; p++) {
        th.emplace_back([&f, p] { f(p); });
    }
    f(0);
    for (auto &t : th) {
        t.join();
    }
}

/* per-read host loops of the read-set steps (geometry from the CIGARs, event candidates): independent reads, split
 * over a few threads when there are enough of them.  f(begin, end, part) */
template <typename F>
static void lfq_for_reads(int64_t n, F f, int *parts_out = nullptr)
{
    int parts = 1;
    const int64_t par_min = lfq_knobs().host_par_min;        /* LFQ_HOST_PAR_MIN (200000): below it one thread does it */
    if (n >= par_min) {
        unsigned hw = lfq_cpu_budget();
        hw = std::max(1u, hw / (unsigned)lfq_knobs().local_world_size);
        const unsigned want = (unsigned)std::min<long>(std::max<long>(lfq_knobs().host_loop_threads, 1), LFQ_HOST_PARTS);
        parts = (int)std::min<int64_t>(std::min<unsigned>(hw ? hw : 1u, want), n / std::max<int64_t>(par_min / 2, 1));
        parts = std::max(parts, 1);
    }
    if (parts_out) {
        *parts_out = parts;
    }
    lfq_run_parts(parts, [&](int p) { f(n * p / parts, n * (p + 1) / parts, p); });
}

/* what lfq_readset_plp_summary hands out (host arrays, valid until the next summary call on the context) */
struct LfqSummaryOwned {
    lfq_plp_summary sum;
    std::vector<int64_t> col_pos, key_off;
    std::vector<uint8_t> ref_base, cons_kind;
    std::vector<int32_t> n_ins, n_dels, hrun, cov;
    std::vector<char> key_chars;
};

#define LFQ_PIN_SLOTS 40

/* the event pair around the kernels of a timed call, for its lfq_last_*_times getter: created on first use, kept until
 * lfq_destroy.  ms() leaves *out alone before the first begin() and where the runtime has no time to give */
struct LfqEvPair {
    hipEvent_t ev[2];
    int begin(hipStream_t st)
    {
        for (hipEvent_t &e : ev) {
            if (!e && hipEventCreate(&e) != hipSuccess) {
                return LFQ_ERR_HIP;
            }
        }
        return hipEventRecord(ev[0], st) == hipSuccess ? (int)LFQ_OK : (int)LFQ_ERR_HIP;
    }
    int end(hipStream_t st) { return !ev[1] || hipEventRecord(ev[1], st) == hipSuccess ? (int)LFQ_OK : (int)LFQ_ERR_HIP; }
    template <typename T> int ms(T *out) const        /* (the public structs hold float or double milliseconds) */
    {
        float t = 0.f;
        if (ev[1] && hipEventSynchronize(ev[1]) != hipSuccess) {
            return LFQ_ERR_HIP;
        }
        if (ev[1] && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) {
            *out = (T)t;
        }
        return LFQ_OK;
    }
    void destroy()
    {
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
};

/* the table of one name of a BED on the device and on the host (lfq_set_bed, lfq_bed.hip).  The context holds one reference, every
 * read set created while it was set another: a later lfq_set_bed leaves the read sets of the earlier one as they are */
struct LfqBedDev {
    std::atomic<int> refs;
    LfqBedName host;
    int32_t *d;                         /* beg[n] | pmax[n] */
    LfqBedTab tab;                      /* ... as the kernels take them */
};
static inline LfqBedDev *lfq_bed_dev_retain(LfqBedDev *b)
{
    if (b) b->refs.fetch_add(1);
    return b;
}
void lfq_bed_dev_release(LfqBedDev *b);    /* lfq_bed.hip */

struct lfq_ctx {
    int device;
    hipStream_t stream;
    LfqLuts *d_luts;
    /* per-batch workspace, grown on demand */
    int64_t ws_cols;
    uint8_t *d_flags;
    uint8_t *d_approx_mu;      /* -t: one double per column of a segment (lfq_launch_approx_gate), grow-only */
    int64_t approx_mu_bytes;
    int32_t *d_prefix, *d_counters;
    LfqEntry *d_entries;
    hipStream_t dps;           /* scan + light DP of a segment, beside the next segment's count kernel */
    hipStream_t side[2];       /* big / mid DP kernels run beside the light one */
    hipEvent_t ev_mid;
    hipEvent_t ev_cnt[LFQ_MAX_SEGMENTS][2];    /* count kernel of segment s: start, stop (main stream) */
    hipEvent_t ev_scan[LFQ_MAX_SEGMENTS];      /* work lists of segment s ready (dps) */
    hipEvent_t ev_light[LFQ_MAX_SEGMENTS][2];  /* light kernel (dps) */
    hipEvent_t ev_side[2][LFQ_MAX_SEGMENTS][2];/* big / mid kernels (side streams) */
    hipEvent_t ev_join[3];
    int cur_segments;
    uint64_t *d_tiles;
    double *d_scratch;
    int64_t scratch_doubles;
    LfqLong *d_longs;             /* row-split columns (lfq_internal.h) */
    LfqSegCell *d_pool;
    int32_t long_cap, pool_cells;
    hipEvent_t ev_segw, ev_prep;
    int32_t *d_unsplit;
    uint8_t *d_retry;          /* light columns the quad kernel hands to the one-column-per-wave kernel */
    int32_t *h_counters;   /* pinned */
    /* layer-2 owned outputs / staging */
    lfq_col_counts *d_counts;
    int64_t counts_cap;
    lfq_col_pvals *d_pvals;
    int64_t pvals_cap;
    uint8_t *d_stage;
    int64_t stage_bytes;
    /* state of the batch in flight */
    hipStream_t cur_stream;
    int64_t cur_pvals_cap;
    int64_t cur_ncols;
    hipEvent_t ev[4];
    lfq_kernel_times times;
    lfq_dp_work work;
    int64_t cur_count_read, cur_count_written;   /* layout bytes of this batch's count kernel (lfq_dp_work) */
    const uint64_t *cur_col_off;                 /* device: CSR offsets of the batch in flight */
    int cur_obs_bytes_x2, cur_col_bytes;
    int cur_sparse_counts;           /* this batch's count kernel stored the dense entries of the tested columns only */
    int n_cu;
    /* strand-bias precompute (lfq_internal.h): DP4 tuples land in host-mapped memory right after the scan;
     * a leader thread waits for that and runs the Fisher tests on the host pool while the DP kernels run */
    int32_t *h_tuples, *d_tuples_mapped;      /* [3 * heavy_cap][4] */
    int32_t *h_nheavy, *d_nheavy_mapped;
    int heavy_cap;
    hipEvent_t ev_heavy;
    uint8_t *d_plp_in, *d_plp_out;   /* device-side pileup: inputs + counters, and the tracks handed out (grow-only:
                                      * hipMalloc / hipFree of gigabytes per region cost milliseconds each) */
    int64_t plp_in_bytes, plp_out_bytes;
    uint8_t *d_tmp[5];               /* grow-only temporaries: BAQ geometry, indel counters, gathers, and the event-read
                                      * arrays + pseudo-column tracks of lfq_call_indels_batch */
    /* the allocations of the read set destroyed last (reads, tags, read ends, tag flags, pinned flags): the next
     * lfq_readset_create / _baq takes them over when they are large enough -- a worker goes from region to region, and
     * hipMalloc + hipFree of 2 GB per region are milliseconds and a device synchronisation each */
    struct { void *p; size_t cap; } rs_cache[9];
    int priv_stream_on;
    hipStream_t priv_stream;         /* lfq_set_private_stream: this context's own launch stream (null = the device's shared one) */
    hipStream_t up_stream;           /* lfq_readset_create's uploads and the staging copies of host tracks (created on first use) */
    hipEvent_t ev_up;                /* end of the staging copies of a batch of host tracks */
    hipEvent_t ev_apply;             /* lfq_readset_pileup_snv: the column positions are final (created on first use) */
    uint8_t *h_pin;                  /* pinned host staging of the BAQ geometry + launch order (grow-only: grow_pinned, as the three below) */
    int64_t pin_bytes;
    uint8_t *h_pin2;                 /* pinned landing area of the indel pileup's per-position counters (grow-only) */
    int64_t pin2_bytes;
    int64_t tmp_bytes[5];
    int64_t plp_ne_cap;              /* capacity of d_plp_ne in int16 elements */
    LfqIndelColsOwned *plp_indel;
    int indel_host_arrays;           /* lfq_set_indel_arrays_on_host */
    int16_t *d_plp_ne;               /* quality arrays of the columns above, resident: [q0 | mq0 | q1 | mq1] */
    int64_t plp_ne_total[2];
    int dense_counts;                /* lfq_set_dense_counts: 0 = a caller's dense array may keep stale entries for untested columns */
    int dense_strand;                /* lfq_set_dense_strand_counts: layer 1 / async layer 2 fill the strand fields of every dense entry */
    int lazy_forced;                 /* set by lfq_call_snvs_batch around its submit */
    LfqEvPair baq_t;                 /* around the BAQ kernels of the last lfq_readset_baq / lfq_baq_batch call */
    int32_t baq_launches;            /* kernel launches between them on the context's stream */
    int64_t baq_reads, baq_bases;    /* reads / bases of that call */
    LfqEvPair fill_t;                /* around the merge pass of the last lfq_readset_baq_fill call */
    lfq_baq_fill_stats fill_stats;   /* counts and launches of that call (the ms: from the events, when asked for) */
    int fill_hmm, fill_merge;        /* that call ran the HMM (ms_hmm comes from baq_t) / the merge pass */
    LfqEvPair idq_t;                 /* around the kernels of the last lfq_readset_indelqual / lfq_indelqual_batch call */
    lfq_indelqual_times idq_times;   /* launches, reads and bases of that call (ms_kernels: from the events, when asked for) */
    int batch_gate;                  /* lfq_set_batch_gate: what this context's next count kernel waits for (LFQ_GATE_*) */
    int lazy_now;                    /* this batch: strand counts only for the columns of the sparse output */
    int64_t sub_ncols;               /* batch submitted with lfq_call_snvs_submit and not collected yet: its columns, else -1 */
    int batch_recorded;              /* ev[3] has been recorded: a batch of this context may still be running */
    float baq_par_d, baq_par_e;      /* lfq_set_baq_hmm_params; kpa_ext_par_lofreq_illumina (kprobaln_ext.c:50) by default */
    int plp_nt_bytes;                /* lfq_set_pileup_nt_packed(ctx, 0): the device pileup hands out one nt byte per observation */
    int plp_unsorted_ok;             /* lfq_set_pileup_unsorted(ctx, 1): reads that are not position-sorted go to the read-major kernels
                                      * instead of being refused (a column's observations then arrive in no fixed order) */
    int64_t plp_max_depth;           /* lfq_set_max_depth: mpileup's -d cap on the reads (LFQ_NO_MAX_DEPTH = none) */
    const uint8_t *sub_ref_host;
    double sub_t0, sub_t1;
    const float *detlim_af;          /* device: per-column allele frequency while lfq_uniq_detlim_batch runs, else null */
    float *d_detlim;
    int64_t detlim_cap;
    int32_t *d_plp_nb;               /* num_bases of the tracks last handed out, and their column count */
    /* lfq_readset_pileup_sites / lfq_readset_uniq: site list, windows, counts and keys; the tracks handed out (both grow-only, and
     * not d_plp_in / d_plp_out: the region pileup's tracks stay as they are) */
    uint8_t *d_sites_in, *d_sites_out;
    int64_t sites_in_bytes, sites_out_bytes;
    LfqEvPair sites_t[2];            /* around the count pass, around the scatter pass */
    lfq_sites_times sites_times;     /* sites, observations and launches of the last call (the ms: from the events, when asked for) */
    int64_t plp_ncols;
    /* lfq_readset_plp_summary: column list, increment table and the kernel's output (grow-only); the host arrays handed out */
    uint8_t *d_sum;
    int64_t sum_bytes;
    uint8_t *h_sum;                  /* pinned: what the kernel wrote (fw | rv | heads | tails | consensus letter | path), handed out as it lies */
    int64_t h_sum_bytes;
    struct LfqSummaryOwned *plp_sum;
    LfqEvPair sum_t;                 /* around the summary kernel */
    lfq_summary_times sum_times;     /* columns, ordered columns and launches of the last call (the ms: from the events, when asked for) */
    /* lfq_plp_quals_from_tracks: the uploaded slice of host tracks | the kernel's output (grow-only); its pinned copy, handed out */
    uint8_t *d_pq;
    int64_t pq_bytes;
    uint8_t *h_pq;                   /* pinned: nt_off | bq | baq | mq | sq as the kernel wrote them */
    int64_t h_pq_bytes;
    lfq_plp_quals plp_quals;         /* the struct handed out */
    LfqEvPair pq_t;                  /* around the group kernel */
    lfq_plp_quals_times pq_times;    /* columns, observations and launches of the last call (the ms: from the events, when asked for) */
    int indel_all_columns;           /* lfq_set_indel_arrays_all_columns */
    /* BAQ scratch (lfq_baq_batch), kept between calls */
    double *d_baq_scr;
    int32_t *d_baq_expect;
    uint8_t *d_baq_tmp8;
    uint8_t *d_baq_nflag;            /* one byte per wavefront of the plain narrow-band launches: the wavefront meets an N */
    int64_t baq_nflag_bytes;
    int32_t *d_baq_itab;
    double *d_baq_terms;
    int64_t baq_scr_bytes, baq_expect_bytes, baq_tmp8_bytes, baq_itab_bytes, baq_terms_bytes;
    std::thread *leader;
    std::mutex *lm;
    std::condition_variable *lcv;
    int leader_go, leader_stop;
    int own_streams;                 /* holds a reference on the device's shared streams */
    int kreg_hint, kreg_hint_indel;  /* screen-kernel variant for the next SNV / indel batch: from the last batch's K histogram */
    int cur_indel_mode;
    int sb_pending;                  /* strand-bias precomputes of this context not finished yet (under lm) */
    struct { void *p; size_t cap; int used; } pin_pool[LFQ_PIN_SLOTS];   /* LfqPin: pinned host temporaries */
    struct LfqViterbiState *vit;     /* lfq_viterbi_batch: its result and device buffers (lfq_viterbi.hip; created on first use) */
    struct LfqBamState *bam;         /* lfq_readset_create_from_bam / _encode_bam: records, descriptors, results and timing (lfq_bamrec.hip; created on first use) */
    struct LfqBgzfState *bgzf;       /* lfq_bgzf_inflate: its buffers, result and timing (lfq_bgzf.hip; created on first use) */
    struct LfqBgzfDefState *bgzf_def; /* lfq_bgzf_deflate: likewise (lfq_bgzf_deflate.hip) */
    struct LfqBamIdxState *bamidx;   /* lfq_bam_index_build: likewise (lfq_bamidx.hip) */
    LfqBedDev *bed;                  /* lfq_set_bed: the targets the read sets created from now on take (null: none) */
    struct LfqFastaState *fasta;     /* lfq_fasta_*: timing and the live fetch result (lfq_fasta.hip; created on first use) */
    struct LfqVcfState *vcf;         /* lfq_vcf_* / lfq_vcfset: timing and the last vcfset result (lfq_vcf.hip; created on first use) */
};

template <typename T>
int grow(T **ptr, int64_t *cap, int64_t need)
{
    if (need <= *cap && *ptr) {
        return LFQ_OK;
    }
    if (*ptr) {
        (void)hipFree(*ptr);
        *ptr = nullptr;
    }
    int64_t n = std::max<int64_t>(need, 16);
    if (hipMalloc((void **)ptr, (size_t)n * sizeof(T)) != hipSuccess) {
        *cap = 0;
        return LFQ_ERR_NOMEM;
    }
    *cap = n;
    return LFQ_OK;
}

/* ... and the same contract for a pinned host block (what a copy from the device lands in, or one to it starts from) */
static inline int grow_pinned(uint8_t **ptr, int64_t *cap, int64_t need)
{
    if (need <= *cap && *ptr) {
        return LFQ_OK;
    }
    if (*ptr) {
        (void)hipHostFree(*ptr);
        *ptr = nullptr;
    }
    if (hipHostMalloc((void **)ptr, (size_t)std::max<int64_t>(need, 16), hipHostMallocDefault) != hipSuccess) {
        *cap = 0;
        return LFQ_ERR_NOMEM;
    }
    *cap = std::max<int64_t>(need, 16);
    return LFQ_OK;
}
static inline void free_pinned(uint8_t **ptr, int64_t *cap)
{
    if (*ptr) (void)hipHostFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
}

/* is `p` pinned (or registered) host memory?  The runtime copies from such memory by DMA and hipMemcpyAsync returns at once */
static inline bool lfq_is_pinned(const void *p)
{
    if (!p) {
        return true;                        /* nothing to copy */
    }
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();            /* plain malloc'ed memory: an error, by design of that call */
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

/* Host temporaries a DMA reads or writes come from a grow-only pool of pinned blocks owned by the context (lfq_api.hip) */
void *lfq_pin_acquire(lfq_ctx *c, size_t bytes, int *slot);

template <typename T>
struct LfqPin {
    lfq_ctx *c;
    T *p = nullptr;
    size_t n = 0;
    int slot = -1;
    LfqPin(lfq_ctx *ctx, size_t count) : c(ctx), n(count)
    {
        p = (T *)lfq_pin_acquire(c, std::max<size_t>(count, 1) * sizeof(T), &slot);
    }
    LfqPin(lfq_ctx *ctx, size_t count, T v) : LfqPin(ctx, count)
    {
        if (p) {
            std::fill(p, p + n, v);
        }
    }
    LfqPin(const LfqPin &) = delete;
    LfqPin &operator=(const LfqPin &) = delete;
    ~LfqPin()
    {
        if (slot >= 0) {
            c->pin_pool[slot].used = 0;
        }
    }
    bool ok() const { return p != nullptr; }
    T *data() { return p; }
    const T *data() const { return p; }
    size_t size() const { return n; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    T &back() { return p[n - 1]; }
};
#define LFQ_PIN_OK(v)                                                                                                  \
    do {                                                                                                               \
        if (!(v).ok()) {                                                                                               \
            return LFQ_ERR_NOMEM;                                                                                      \
        }                                                                                                              \
    } while (0)

/* ---- internal functions that cross file boundaries (lfq_api.hip) ---- */
int lfq_make_params(const lfq_conf *conf, const lfq_tracks *tr, LfqParams *P, bool indel_mode);
void lfq_viterbi_release(lfq_ctx *c);      /* lfq_viterbi.hip: what lfq_destroy frees of lfq_ctx::vit */
/* lfq_viterbi_batch; with `res` (lfq_readset_viterbi: the device view of a read set whose host arrays are the `reads` of the call),
 * query, q2def and windows are gathered on the device instead of packed and uploaded */
int lfq_viterbi_run(lfq_ctx *c, const lfq_baq_reads *reads, int def_qual, const LfqReadsDev *res,
                    const lfq_viterbi_result **out);
/* dst[k][new order] = src[k][old order] for up to four per-base arrays; returns when the kernel is done */
int lfq_viterbi_permute(lfq_ctx *c, int64_t n_reads, int64_t n_bases, const int64_t *d_new_off, const int64_t *old_start,
                        int n_arrays, const uint8_t *const *src, uint8_t *const *dst);
/* lfq_bamrec.hip.  The records of an lfq_bam_records as both calls send them down (lfq_readset.hip builds it once per call) */
struct LfqBamIn {
    const uint8_t *data;                /* the first record's first byte */
    int64_t data_bytes;                 /* ... to the last record's end */
    int first_shift;                    /* data & 15: the room in front of the records on the device, so that a record keeps the
                                           alignment it has in the caller's memory */
    bool pinned;                        /* data lies in pinned host memory: no staging copy */
};
/* for lfq_readset_create_from_bam (lfq_readset.hip): upload + aux pass, then the base pass into a read set's device arrays and the
 * copies back; both block */
void lfq_bam_release(lfq_ctx *c);
void lfq_bam_times_reset(lfq_ctx *c, int64_t n_reads, int64_t n_bases, int64_t n_data_bytes);
int lfq_bam_aux(lfq_ctx *c, const LfqBamIn &in, const int64_t *desc, int64_t n, int64_t nb, uint8_t *flags_out, int *any_bi,
                int *any_bd, unsigned read_tags, uint8_t *stored_out);
int lfq_bam_bases(lfq_ctx *c, uint8_t *d_seq, uint8_t *d_qual, uint8_t *d_bi, uint8_t *d_bd, uint8_t *h_seq, uint8_t *h_qual,
                  uint8_t *h_bi, uint8_t *h_bd);
/* for lfq_readset_create_from_bam_tags / lfq_readset_baq_fill (lfq_readset.hip): the stored-tag pass of the decode in flight into
 * the side arrays (null: no read has the tag; blocks), and the merge pass queued on `st`: per read r and tag t (lb, ai, ad) with bit
 * t of d_take[r], the bytes of src[t] replace those of dst[t]; with d_tagfl the ai / ad bits are ORed into it */
int lfq_bam_stored(lfq_ctx *c, uint8_t *const d_dst[3]);
int lfq_bam_merge(const int64_t *d_seq_off, const uint8_t *d_take, const uint8_t *const d_src[3], uint8_t *const d_dst[3],
                  uint8_t *d_tagfl, int64_t n, int64_t nb, hipStream_t st);
/* for lfq_readset_encode_bam (lfq_readset.hip): the records rewritten on the device.  One LfqBamRead per read of the read set, in
 * its order; rec / end are offsets from data - first_shift, as for the decode */
struct LfqBamRead {
    int64_t rec, end;                   /* the read's record: its first byte (read_name) and one past its last */
    int32_t l_qseq;
    uint32_t n_cigar;                   /* the record's own */
    uint16_t l_qname, flag;
    uint32_t pad_;
};
struct LfqBamEncIn {
    LfqBamIn recs;
    const LfqBamRead *reads;            /* [n] */
    int64_t n;
    unsigned what;                      /* LFQ_BAM_* */
    bool uniform;                       /* PUT_INDELQUAL: the read set's indel qualities are uniform ones */
    /* the read set's device arrays (of rd: offsets and CIGARs); lb / ai / ad / bi / bd null where `what` does not ask for them */
    LfqReadsDev rd;
    const uint8_t *d_fl, *d_lb, *d_ai, *d_ad, *d_bi, *d_bd;
    /* [n] what the result hands out beside the blob (copied) */
    const int64_t *src;
    const int32_t *pos;
    const uint32_t *n_cigar;
};
int lfq_bam_encode(lfq_ctx *c, const LfqBamEncIn *in, const lfq_bam_encoded **out);
int lfq_bam_encode_empty(lfq_ctx *c, const lfq_bam_encoded **out);
/* lfq_bgzf.hip.  What lfq_destroy frees of lfq_ctx::bgzf; and for bam_upload (lfq_bamrec.hip): the device address of host bytes
 * [p, p + bytes) when they lie inside the context's live inflate result (counted as a decode from the device), else null */
void lfq_bgzf_release(lfq_ctx *c);
const uint8_t *lfq_bgzf_resident(lfq_ctx *c, const uint8_t *p, int64_t bytes);
/* the same address without the count: for lfq_bgzf_deflate (lfq_bgzf_deflate.hip), which keeps its own; its twin for the live
 * lfq_bam_frame_encoded result (lfq_bamrec.hip); and what lfq_destroy frees of lfq_ctx::bgzf_def */
const uint8_t *lfq_bgzf_resident_bytes(lfq_ctx *c, const uint8_t *p, int64_t bytes);
const uint8_t *lfq_bam_framed_resident(lfq_ctx *c, const uint8_t *p, int64_t bytes);
void lfq_bgzf_deflate_release(lfq_ctx *c);
void lfq_bam_index_release(lfq_ctx *c);    /* lfq_bamidx.hip: what lfq_destroy frees of lfq_ctx::bamidx */
/* lfq_bamidx.hip: the compaction its build shares with lfq_vcf_index_build (lfq_tbx.hip).  reserve lays out, in the context's grow-only
 * buffer, head_bytes of the caller's own, n_recs LfqBaiRec and the compaction's lists; the caller's record pass fills rec[] and sets
 * counters[0 .. 4) (0: its own word, 1 .. 3: zero); compact launches the part / scan / emit kernels on the context's stream and brings
 * chunks, runs and intervals to pinned host memory, valid until the context's next reserve.  lfq_bai_vcf_times: where
 * lfq_last_vcf_index_times reads, freed with the rest of lfq_ctx::bamidx */
struct LfqBaiRec;
struct LfqBaiChunk;
struct LfqBaiRun;
struct LfqBaiIntv;
struct LfqBaiDev {
    uint8_t *head;
    LfqBaiRec *rec;
    unsigned long long *counters;
};
struct LfqBaiLists {
    const LfqBaiChunk *chunks;
    const LfqBaiRun *runs;
    const LfqBaiIntv *intvs;
    int64_t n_chunks, n_runs, n_intvs;
    double kernels_ms, download_ms;
};
int lfq_bai_reserve(lfq_ctx *c, int64_t head_bytes, int64_t n_recs, int64_t max_runs, LfqBaiDev *out);
int lfq_bai_compact(lfq_ctx *c, LfqBaiLists *out);
lfq_vcf_index_times *lfq_bai_vcf_times(lfq_ctx *c);
/* lfq_fasta.hip.  What lfq_destroy frees of lfq_ctx::fasta; and for the read set's contig upload (lfq_readset.hip): the device address
 * of host bytes [p, p + bytes) when they lie inside the context's live lfq_fasta_fetch result (counted as a hand-over), else null */
void lfq_fasta_release(lfq_ctx *c);
const uint8_t *lfq_fasta_resident(lfq_ctx *c, const uint8_t *p, int64_t bytes);
void lfq_vcf_release(lfq_ctx *c);          /* lfq_vcf.hip: what lfq_destroy frees of lfq_ctx::vcf */
/* lfq_vcf.hip, for lfq_tbx.hip: an open file's context, mode, table on the device and run names */
struct LfqVcTab;
void lfq_vcf_view(const lfq_vcf *v, lfq_ctx **c, int *mode, LfqVcTab *T, const std::vector<std::string> **names);
/* lfq_bed.hip, for the read set (lfq_readset.hip).  keep_out[r] = 1 iff [pos, bam_endpos) of read r overlaps an interval, one lane
 * per read, from the resident start positions and CIGAR words; cov[p] (and nb[p], unless null) of every position of
 * [begin, begin + width) whose [p, p + 1) overlaps none go to 0, one lane per position: no column for the compaction behind it */
int lfq_launch_bed_keep(const LfqBedTab &tab, const int32_t *pos, const int64_t *cigar_off, const uint32_t *cigar, int64_t n,
                        uint8_t *keep_out, void *stream);
int lfq_launch_bed_mask_columns(const LfqBedTab &tab, int64_t begin, int64_t width, int32_t *cov, int32_t *nb_or_null, void *stream);
extern "C" {
/* everything the library queues that rewrites what a running batch still reads waits for the batch's last event first */
int lfq_order_after_batch(lfq_ctx *c, hipStream_t st);
int lfq_batch_device_impl(lfq_ctx *c, const lfq_conf *conf, const lfq_tracks *tr, lfq_col_counts *d_counts,
                          lfq_col_pvals *d_pvals, int64_t pvals_capacity, void *stream_or_null, bool indel_mode);
int lfq_stage_tracks(lfq_ctx *c, const lfq_tracks *tr, int tracks_on_device, lfq_tracks *dev_out);
/* lfq_readset_pileup_sites (lfq_readset.hip), with the event match of lfq_readset_uniq: key_off null = no keys; ev_out gets the
 * matching entries per site */
int lfq_readset_sites_impl(lfq_ctx *c, lfq_readset *rs, const int64_t *site_pos, int64_t n_sites, int min_plp_bq,
                           const int64_t *key_off, const char *key_chars, const uint8_t *key_del, lfq_tracks *out,
                           int32_t *cov_out, int32_t *nb_out, int32_t *tails_out, int32_t *ev_out);
/* lfq_readset_create_from_bam_tags with records that do not abut: record r ends at data_end[r] <= data_off[r + 1] (null: at
 * data_off[r + 1]).  lfq_readset.hip, for lfq_readset_create_from_bgzf (lfq_bgzf.hip) */
int lfq_readset_from_bam_ends(lfq_ctx *c, const lfq_bam_records *recs, const int64_t *data_end, unsigned read_tags, lfq_readset **out);
}

#endif
