/*
 * lfq_plp_indel_host.h -- the host half of the indel pileup (lfq_readset_pileup_indels, lfq_readset.hip) as plain C++: events
 * from the CIGARs, the event tables, the columns from the kernel's nine per-position counters, the consensus indel, the arrays
 * handed out.  No HIP, no context, no knobs, no threads: every stage names what it reads and writes, those that are split over
 * threads take their range or part, and the caller runs them (lfq_plp_indel_host_check.cpp: on the host, one after the other). */
#ifndef LFQ_PLP_INDEL_HOST_H
#define LFQ_PLP_INDEL_HOST_H

#include <ctype.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "lfq_internal.h"

/* std::vector whose resize() leaves new elements of a trivial type uninitialised: the per-region column arrays (tens of MB)
 * are resized by one thread and then written in full by the pool's threads -- value-initialising them first was a serial
 * memset of every array, milliseconds per region. */
template <class T>
struct LfqNoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { typedef LfqNoInitAlloc<U> other; };
    LfqNoInitAlloc() = default;
    template <class U> LfqNoInitAlloc(const LfqNoInitAlloc<U> &) {}
    template <class U> void construct(U *p) { ::new ((void *)p) U; }
    template <class U, class A0, class... Args> void construct(U *p, A0 &&a0, Args &&...args)
    {
        ::new ((void *)p) U(std::forward<A0>(a0), std::forward<Args>(args)...);
    }
};
template <class T> using LfqVec = std::vector<T, LfqNoInitAlloc<T>>;

/* the columns handed out by lfq_pileup_indel_columns live here until the next call */
struct LfqIndelColsOwned {
    lfq_indel_columns cols;
    LfqVec<uint8_t> ref_base, cons_indel;
    LfqVec<int32_t> cov, tails, non_indels, n_ins, n_dels, hrun;
    std::vector<int32_t> ne_qsum[2];     /* per column: ins_nonevent_qual / del_nonevent_qual (plp.c:810) where the column-major kernel summed them */
    struct Side {
        LfqVec<int32_t> non_fw, non_rv, ev_fw, ev_rv;
        LfqVec<int64_t> ne_off, ev_off, key_off, rd_off;
        LfqVec<int16_t> ne_q, ne_mq, rd_q, rd_aq, rd_mq, rd_sq;
        LfqVec<char> key_chars;
    } side[2];
    void reset()
    {
        memset(&cols, 0, sizeof(cols));
        ref_base.clear(); cons_indel.clear();
        cov.clear(); tails.clear(); non_indels.clear(); n_ins.clear(); n_dels.clear(); hrun.clear();
        ne_qsum[0].clear(); ne_qsum[1].clear();
        for (Side &s : side) {
            s.non_fw.clear(); s.non_rv.clear(); s.ev_fw.clear(); s.ev_rv.clear();
            s.ne_off.clear(); s.ev_off.clear(); s.key_off.clear(); s.rd_off.clear();
            s.ne_q.clear(); s.ne_mq.clear(); s.rd_q.clear(); s.rd_aq.clear(); s.rd_mq.clear(); s.rd_sq.clear();
            s.key_chars.clear();
        }
    }
};

/* the host arrays of the reads the stages below look at (an lfq_readset's, filled in one place) */
struct LfqPlpReads {
    const int32_t *pos;
    const int64_t *cigar_off, *seq_off;
    const uint32_t *cigar;
    const uint8_t *seq, *mapq, *reverse;
    const char *ref; int64_t ref_len;
    const uint8_t *bi, *bd, *ai, *ad;   /* tag bytes per base where the caller gave them (may be null) */
    const uint8_t *fl;                  /* per read: bit 0..3 = has BI / BD / ai / ad (ai / ad: valid once the BAQ kernels are through) */
    const int32_t *sq;                  /* source quality per read, or null */
    int idq_mode; uint8_t idq_ins, idq_del;     /* BI / BD computed by lfq_readset_indelqual: evaluated for the event's base, not read */
    const uint8_t *keep;                /* [n] 0 = dropped by the -d cap: in no column; null = every read */
};

/* the reference base of a column, plp.c:818-823 */
static inline uint8_t lfq_plp_ref_base(const char *ref, int64_t ref_len, int64_t pos)
{
    const uint8_t rb = (ref && pos < ref_len) ? (uint8_t)ref[pos] : (uint8_t)'N';
    return (rb == 'A' || rb == 'C' || rb == 'T' || rb == 'G') ? rb : (uint8_t)'N';
}

/* BI (q[0]) and BD (q[1]) of query base qpos of read r as qualities; 0 where the read has no such tag (or no base) */
static inline void lfq_plp_idq(const LfqPlpReads &R, int64_t r, int qpos, int *q)
{
    if (qpos < 0) {
        q[0] = q[1] = 0;
    } else if (R.idq_mode == LFQ_IDQ_UNIFORM) {
        q[0] = (int)R.idq_ins - 33;
        q[1] = (int)R.idq_del - 33;
    } else if (R.idq_mode) {
        q[0] = q[1] = (int)lfq_idq_host_byte(R.ref, R.ref_len, R.pos[r], R.cigar + R.cigar_off[r],
                                             (int)(R.cigar_off[r + 1] - R.cigar_off[r]), qpos) - 33;
    } else {
        const int64_t b = R.seq_off[r] + qpos;
        q[0] = (R.bi && (R.fl[r] & 1u)) ? (int)R.bi[b] - 33 : 0;
        q[1] = (R.bd && (R.fl[r] & 2u)) ? (int)R.bd[b] - 33 : 0;
    }
}

/* ---- 1. events from the CIGARs, in read (= pileup) order ---- */
struct LfqPlpEv { int64_t pos; int64_t read; int32_t qpos, indel; };
static inline bool lfq_plp_ev_before(const LfqPlpEv &a, const LfqPlpEv &b) { return a.pos < b.pos; }

/* the events of the reads [r_begin, r_end) inside [region_begin, region_end), appended to evs and sorted by position, those
 * of one position in read order */
static inline void lfq_plp_scan_events(const LfqPlpReads &R, int64_t r_begin, int64_t r_end, int64_t region_begin,
                                       int64_t region_end, int min_plp_idq, std::vector<LfqPlpEv> &evs)
{
    for (int64_t r = r_begin; r < r_end; r++) {
        if (R.keep && !R.keep[r]) {
            continue;
        }
        const uint32_t *cg = R.cigar + R.cigar_off[r];
        const int n_cigar = (int)(R.cigar_off[r + 1] - R.cigar_off[r]);
        const int l_qseq = (int)(R.seq_off[r + 1] - R.seq_off[r]);
        int64_t x = R.pos[r];
        int y = 0;
        for (int k = 0; k < n_cigar; ++k) {
            const int op = cg[k] & 0xf, l = cg[k] >> 4;
            if (op == 0 || op == 7 || op == 8 || op == 2 || op == 3) {
                const bool is_del = op == 2 || op == 3;
                const int indel = l > 0 ? lfq_cigar_peek_indel(cg, n_cigar, k) : 0;
                const int64_t p = x + l - 1;
                if (indel != 0 && p >= region_begin && p < region_end) {
                    int qpos = is_del ? y : y + l - 1, q[2];
                    qpos = qpos < l_qseq ? qpos : l_qseq - 1;
                    lfq_plp_idq(R, r, qpos, q);
                    if (!(q[0] < min_plp_idq || q[1] < min_plp_idq)) {      /* plp.c:1062 */
                        evs.push_back({p, r, qpos, indel});
                    }
                }
                x += l;
                if (!is_del) {
                    y += l;
                }
            } else if (op == 1 || op == 4) {
                y += l;
            }
        }
    }
    std::stable_sort(evs.begin(), evs.end(), lfq_plp_ev_before);
}

/* ... and the parts, which are consecutive ranges of position-sorted reads and overlap only at their ends, are merged
 * one after the other (std::inplace_merge keeps equal positions in part order = read order) */
static inline void lfq_plp_merge_events(const std::vector<LfqPlpEv> *parts, int n_parts, std::vector<LfqPlpEv> &evs)
{
    for (int p = 0; p < n_parts; p++) {
        const size_t mid = evs.size();
        evs.insert(evs.end(), parts[p].begin(), parts[p].end());
        if (mid > 0 && mid < evs.size() && lfq_plp_ev_before(evs[mid], evs[mid - 1])) {
            /* (only the tail of what is there can lie behind the new part's first event) */
            const auto first = std::upper_bound(evs.begin(), evs.begin() + (std::ptrdiff_t)mid, evs[mid], lfq_plp_ev_before);
            std::inplace_merge(first, evs.begin() + (std::ptrdiff_t)mid, evs.end(), lfq_plp_ev_before);
        }
    }
}

/* ---- 4. event tables: per column and side, events in order of first appearance (uthash iterates in insertion order), their
 * reads in pileup order (add_ins_sequence / add_del_sequence, utils.c).  Columns with events are few and independent of one
 * another: the event list is cut at position boundaries into a few parts, every part builds the tables of its columns, and the
 * parts are appended in order ---- */
struct LfqPlpPartTables {
    LfqIndelColsOwned::Side side[2];        /* key_off / rd_off: local running totals, no leading 0 */
    std::vector<int64_t> cols;              /* positions (relative to the region) with events, ascending */
    std::vector<int64_t> ev_after[2];       /* local event count of each side after each of them */
    std::vector<int64_t> rd_ev[2];          /* event index of each entry of side[sd].rd_q (for rd_aq, filled last) */
};

/* part t = events [cut[t], cut[t + 1]): even shares, moved on so that no position is split */
static inline std::vector<size_t> lfq_plp_table_cuts(const std::vector<LfqPlpEv> &evs, int n_parts)
{
    std::vector<size_t> cut((size_t)n_parts + 1, evs.size());
    cut[0] = 0;
    for (int t = 1; t < n_parts; t++) {
        size_t k = evs.size() * (size_t)t / (size_t)n_parts;
        while (k < evs.size() && k > 0 && evs[k].pos == evs[k - 1].pos) {
            k++;
        }
        cut[(size_t)t] = std::max(k, cut[(size_t)t - 1]);
    }
    return cut;
}

static inline void lfq_plp_build_tables(const LfqPlpReads &R, const std::vector<LfqPlpEv> &evs, size_t e_begin, size_t e_end,
                                        int64_t region_begin, LfqPlpPartTables &P)
{
    std::vector<std::string> keys;
    std::vector<std::vector<size_t>> members;
    std::string key;
    for (size_t ei = e_begin, e1; ei < e_end; ei = e1) {
        for (e1 = ei; e1 < e_end && evs[e1].pos == evs[ei].pos; e1++) {
        }
        P.cols.push_back(evs[ei].pos - region_begin);   /* the position; its column index is known once the counters are back */
        for (int sd = 0; sd < 2; sd++) {
            LfqIndelColsOwned::Side &S = P.side[sd];
            keys.clear();                       /* (reused across columns: no allocation in the common case) */
            for (auto &m : members) {
                m.clear();
            }
            size_t n_keys = 0;
            for (size_t i = ei; i < e1; i++) {
                const LfqPlpEv &e = evs[i];
                if ((e.indel > 0) != (sd == 0)) {
                    continue;
                }
                key.clear();
                if (sd == 0) {                                  /* inserted bases, plp.c:1082-1086 */
                    const int64_t s0 = R.seq_off[e.read], lq = R.seq_off[e.read + 1] - s0;
                    for (int j = 1; j <= e.indel; j++) {
                        const int64_t q = e.qpos + j;
                        key.push_back(lfq_seq_letter(q < lq ? R.seq[s0 + q] : 4));
                    }
                } else {                                        /* deleted reference bases, :1127-1131 */
                    for (int j = 1; j <= -e.indel; j++) {
                        const int64_t g = e.pos + j;
                        key.push_back(g < R.ref_len ? (char)toupper((unsigned char)R.ref[g]) : 'N');
                    }
                }
                size_t ki = 0;
                while (ki < n_keys && keys[ki] != key) {
                    ki++;
                }
                if (ki == n_keys) {
                    keys.push_back(key);
                    if (members.size() <= n_keys) {
                        members.emplace_back();
                    }
                    n_keys++;
                }
                members[ki].push_back(i);
            }
            for (size_t ki = 0; ki < n_keys; ki++) {
                int fw = 0, rv = 0, q[2];
                for (size_t i : members[ki]) {
                    const LfqPlpEv &e = evs[i];
                    lfq_plp_idq(R, e.read, e.qpos, q);
                    S.rd_q.push_back((int16_t)q[sd]);
                    S.rd_aq.push_back((int16_t)-1);                  /* filled when the BAQ kernels are through */
                    P.rd_ev[sd].push_back((int64_t)i);
                    S.rd_mq.push_back((int16_t)R.mapq[e.read]);
                    const int32_t sq = R.sq ? R.sq[e.read] : -1;
                    S.rd_sq.push_back((int16_t)(sq > 32767 ? 32767 : sq));
                    (R.reverse[e.read] ? rv : fw)++;
                }
                S.ev_fw.push_back(fw);
                S.ev_rv.push_back(rv);
                S.key_chars.insert(S.key_chars.end(), keys[ki].begin(), keys[ki].end());
                S.key_off.push_back((int64_t)S.key_chars.size());
                S.rd_off.push_back((int64_t)S.rd_q.size());
            }
            P.ev_after[sd].push_back((int64_t)S.ev_fw.size());
        }
    }
}

/* what the appended parts leave for the later stages: per column with events where its events end on either side, and the
 * event index of each rd_q entry */
struct LfqPlpEvCol { int64_t pos; int64_t ev_after[2]; };
struct LfqPlpTables { std::vector<LfqPlpEvCol> ecols; std::vector<int64_t> rd_ev[2]; };

/* the parts appended to O in order, offsets shifted by what came before (ev_off is filled once the columns are known) */
static inline void lfq_plp_append_tables(const std::vector<LfqPlpPartTables> &pt, LfqIndelColsOwned &O, LfqPlpTables &T)
{
    for (int sd = 0; sd < 2; sd++) {
        O.side[sd].ev_off.push_back(0);
        O.side[sd].key_off.push_back(0);
        O.side[sd].rd_off.push_back(0);
    }
    for (const LfqPlpPartTables &P : pt) {
        int64_t ev_base[2];
        for (int sd = 0; sd < 2; sd++) {
            LfqIndelColsOwned::Side &S = O.side[sd];
            const LfqIndelColsOwned::Side &L = P.side[sd];
            const int64_t rd_base = (int64_t)S.rd_q.size(), key_base = (int64_t)S.key_chars.size();
            ev_base[sd] = (int64_t)S.ev_fw.size();
            S.ev_fw.insert(S.ev_fw.end(), L.ev_fw.begin(), L.ev_fw.end());
            S.ev_rv.insert(S.ev_rv.end(), L.ev_rv.begin(), L.ev_rv.end());
            S.key_chars.insert(S.key_chars.end(), L.key_chars.begin(), L.key_chars.end());
            S.rd_q.insert(S.rd_q.end(), L.rd_q.begin(), L.rd_q.end());
            S.rd_aq.insert(S.rd_aq.end(), L.rd_aq.begin(), L.rd_aq.end());
            S.rd_mq.insert(S.rd_mq.end(), L.rd_mq.begin(), L.rd_mq.end());
            S.rd_sq.insert(S.rd_sq.end(), L.rd_sq.begin(), L.rd_sq.end());
            T.rd_ev[sd].insert(T.rd_ev[sd].end(), P.rd_ev[sd].begin(), P.rd_ev[sd].end());
            for (int64_t v : L.key_off) {
                S.key_off.push_back(v + key_base);
            }
            for (int64_t v : L.rd_off) {
                S.rd_off.push_back(v + rd_base);
            }
        }
        for (size_t i = 0; i < P.cols.size(); i++) {
            T.ecols.push_back({P.cols[i], {ev_base[0] + P.ev_after[0][i], ev_base[1] + P.ev_after[1][i]}});
        }
    }
}

/* ---- 3. columns = covered positions, from the kernel's per-position counters h[0..8] = coverage, tails, non-indels, insertions,
 * deletions, forward reads without an insertion / without a deletion, and (have_qsum) the two non-event quality sums.  Two
 * passes over the positions, both split over a few parts: count the covered positions and the non-event reads at event
 * positions per part, then every part fills its slice of the column arrays ---- */
struct LfqPlpPartCount { int64_t cov, ne[2]; };

/* has_ev[p]: position p of the region gets the quality arrays of its non-event reads (all_columns: every one does) */
static inline void lfq_plp_mark_events(const std::vector<LfqPlpEv> &evs, int64_t region_begin, int64_t width, bool all_columns,
                                       std::vector<uint8_t> &has_ev)
{
    has_ev.assign((size_t)width, all_columns ? 1 : 0);
    for (const LfqPlpEv &e : evs) {
        has_ev[(size_t)(e.pos - region_begin)] = 1;
    }
}

static inline LfqPlpPartCount lfq_plp_cols_count(const int32_t *const *h, const std::vector<uint8_t> &has_ev, int64_t p0, int64_t p1)
{
    LfqPlpPartCount n = {0, {0, 0}};
    for (int64_t p = p0; p < p1; p++) {
        n.cov += h[0][p] > 0;
        if (h[0][p] > 0 && has_ev[(size_t)p]) {
            n.ne[0] += h[2][p] + h[4][p];
            n.ne[1] += h[2][p] + h[3][p];
        }
    }
    return n;
}

/* pc[q + 1] = the counts of part q on entry (pc[0] = 0), what lies before part q + 1 on return; the arrays get their sizes */
static inline void lfq_plp_cols_alloc(LfqIndelColsOwned &O, LfqPlpPartCount *pc, int parts, bool have_qsum)
{
    for (int q = 0; q < parts; q++) {
        pc[q + 1].cov += pc[q].cov;
        pc[q + 1].ne[0] += pc[q].ne[0];
        pc[q + 1].ne[1] += pc[q].ne[1];
    }
    const size_t n_cov = (size_t)pc[parts].cov;
    for (auto *v : {&O.cov, &O.tails, &O.non_indels, &O.n_ins, &O.n_dels, &O.hrun}) {
        v->resize(n_cov);
    }
    O.ref_base.resize(n_cov);
    for (int sd = 0; sd < 2; sd++) {
        if (have_qsum) {
            O.ne_qsum[sd].resize(n_cov);
        }
        O.side[sd].non_fw.resize(n_cov);
        O.side[sd].non_rv.resize(n_cov);
        O.side[sd].ne_off.resize(n_cov + 1);
        O.side[sd].ev_off.reserve(n_cov + 1);
        O.side[sd].ne_off[0] = 0;
    }
}

static inline int lfq_plp_hrun(const char *ref, int64_t ref_len, int64_t gp)       /* get_hrun, plp.c:744-787 */
{
    int hr = 1;
    if (gp + 1 < ref_len) {
        const int ch = toupper((unsigned char)ref[gp + 1]);
        for (int64_t i = gp + 2; i < ref_len && toupper((unsigned char)ref[i]) == ch; i++) {
            hr++;
        }
        for (int64_t i = gp; i >= 0 && toupper((unsigned char)ref[i]) == ch; i--) {
            hr++;
        }
    }
    return hr;
}

/* positions [p0, p1), whose first column and first non-event entries are `before`; col_of[p] = column of an event position (-1:
 * none), pos_off[sd][p] = where the scatter pass puts its non-event reads (-1: nowhere): every position is written */
static inline void lfq_plp_cols_fill(const LfqPlpReads &R, const int32_t *const *h, const std::vector<uint8_t> &has_ev,
                                     int64_t region_begin, int64_t p0, int64_t p1, const LfqPlpPartCount &before, bool have_qsum,
                                     LfqIndelColsOwned &O, int32_t *col_of, int64_t *const *pos_off, int64_t *col_pos_out)
{
    size_t ci = (size_t)before.cov;
    int64_t run[2] = {before.ne[0], before.ne[1]};
    for (int64_t p = p0; p < p1; p++) {
        col_of[p] = -1;
        pos_off[0][p] = pos_off[1][p] = -1;
        if (h[0][p] <= 0) {
            continue;
        }
        const int64_t gp = region_begin + p;
        if (col_pos_out) {
            col_pos_out[ci] = gp;
        }
        O.ref_base[ci] = lfq_plp_ref_base(R.ref, R.ref_len, gp);
        O.cov[ci] = h[0][p];
        O.tails[ci] = h[1][p];
        O.non_indels[ci] = h[2][p];
        O.n_ins[ci] = h[3][p];
        O.n_dels[ci] = h[4][p];
        O.hrun[ci] = lfq_plp_hrun(R.ref, R.ref_len, gp);
        const int32_t ne_cnt[2] = {h[2][p] + h[4][p], h[2][p] + h[3][p]};
        for (int sd = 0; sd < 2; sd++) {
            if (have_qsum) {
                O.ne_qsum[sd][ci] = h[7 + sd][p];
            }
            O.side[sd].non_fw[ci] = h[5 + sd][p];
            O.side[sd].non_rv[ci] = ne_cnt[sd] - h[5 + sd][p];
            if (has_ev[(size_t)p]) {
                pos_off[sd][p] = run[sd];
                run[sd] += ne_cnt[sd];
                col_of[p] = (int32_t)ci;
            }
            O.side[sd].ne_off[ci + 1] = run[sd];
        }
        ci++;
    }
}

/* the running event counts per column (the event-less columns repeat the count before them).  false: an event position is no
 * column (cannot happen: a read with an event covers its position) */
static inline bool lfq_plp_fill_ev_off(const LfqPlpTables &T, const int32_t *col_of, LfqIndelColsOwned &O)
{
    const int64_t ncols = (int64_t)O.cov.size();
    int64_t col_done = 0;                       /* columns [0, col_done) have their ev_off entries */
    for (const LfqPlpEvCol &e : T.ecols) {
        const int64_t col = col_of[e.pos];
        if (col < 0) {
            return false;
        }
        for (int sd = 0; sd < 2; sd++) {
            LfqVec<int64_t> &ev_off = O.side[sd].ev_off;
            ev_off.insert(ev_off.end(), (size_t)(col - col_done), ev_off.back());
            ev_off.push_back(e.ev_after[sd]);
        }
        col_done = col + 1;
    }
    for (int sd = 0; sd < 2; sd++) {            /* the event-less columns behind the last event */
        O.side[sd].ev_off.insert(O.side[sd].ev_off.end(), (size_t)(ncols - col_done), O.side[sd].ev_off.back());
    }
    return true;
}

/* ---- 5. consensus indel (plp.c:1231-1270): of the events [ev_off[col], ev_off[col + 1]) of one side, the first whose sum of
 * qualities is strictly the greatest, if that sum exceeds `non`, the sum over the side's reads without an event; else -1 ---- */
static inline int64_t lfq_plp_cons_event(const int64_t *ev_off, const int64_t *rd_off, const int16_t *rd_q, int64_t col, int64_t non)
{
    int64_t best = std::max<int64_t>(non, 0), best_ev = -1;
    for (int64_t e = ev_off[col]; e < ev_off[col + 1]; e++) {
        int64_t sum = 0;                                    /* cons_quals, utils.c:569, 629 */
        for (int64_t i = rd_off[e]; i < rd_off[e + 1]; i++) {
            sum += rd_q[i];
        }
        if (sum > best) {
            best = sum;
            best_ev = e;
        }
    }
    return best_ev;
}

/* cons_indel of every column: the non-event sums from the kernel (have_qsum) or over the ne_q arrays it scattered */
static inline void lfq_plp_cons_flags(const LfqPlpTables &T, const int32_t *col_of, bool have_qsum, LfqIndelColsOwned &O)
{
    O.cons_indel.assign(O.cov.size(), 0);
    for (const LfqPlpEvCol &e : T.ecols) {
        const int64_t col = col_of[e.pos];
        for (int sd = 0; sd < 2; sd++) {
            const LfqIndelColsOwned::Side &S = O.side[sd];
            int64_t non = have_qsum ? O.ne_qsum[sd][(size_t)col] : 0;
            for (int64_t i = S.ne_off[(size_t)col]; !have_qsum && i < S.ne_off[(size_t)col + 1]; i++) {
                non += S.ne_q[(size_t)i];
            }
            if (lfq_plp_cons_event(S.ev_off.data(), S.rd_off.data(), S.rd_q.data(), col, non) >= 0) {
                O.cons_indel[(size_t)col] = 1;
            }
        }
    }
}

/* ---- 4b. the alignment qualities of the event reads (plp.c:1069-1073, 1113-1117): idx[i] = the base of event i for the gather
 * on the device; then rd_aq from the gathered bytes (g_ai / g_ad, per event) or from the host's ai / ad ---- */
static inline void lfq_plp_gather_index(const LfqPlpReads &R, const std::vector<LfqPlpEv> &evs, int64_t *idx)
{
    for (size_t i = 0; i < evs.size(); i++) {
        idx[i] = R.seq_off[evs[i].read] + evs[i].qpos;
    }
}

static inline void lfq_plp_fill_rd_aq(const LfqPlpReads &R, const std::vector<LfqPlpEv> &evs, const LfqPlpTables &T,
                                      const uint8_t *g_ai, const uint8_t *g_ad, LfqIndelColsOwned &O)
{
    for (int sd = 0; sd < 2; sd++) {
        LfqIndelColsOwned::Side &S = O.side[sd];
        const uint8_t *aa = sd == 0 ? R.ai : R.ad, *ga = sd == 0 ? g_ai : g_ad;
        for (size_t j = 0; j < T.rd_ev[sd].size(); j++) {
            const LfqPlpEv &e = evs[(size_t)T.rd_ev[sd][j]];
            const bool has = (R.fl[e.read] & (sd == 0 ? 4u : 8u)) != 0;      /* no ai / ad tag on this read: -1 */
            if (has && ga) {
                S.rd_aq[j] = (int16_t)((int)ga[(size_t)T.rd_ev[sd][j]] - 33);
            } else if (has && aa) {
                S.rd_aq[j] = (int16_t)((int)aa[R.seq_off[e.read] + e.qpos] - 33);
            }
        }
    }
}

/* ---- 6. publish: the struct handed out points at O's arrays ---- */
static inline void lfq_plp_publish(LfqIndelColsOwned &O)
{
    lfq_indel_columns &C = O.cols;
    C.ncols = (int64_t)O.cov.size();
    C.ref_base = O.ref_base.data(); C.cons_indel = O.cons_indel.data(); C.hrun = O.hrun.data();
    C.coverage_plp = O.cov.data(); C.num_tails = O.tails.data(); C.num_non_indels = O.non_indels.data();
    C.num_ins = O.n_ins.data(); C.num_dels = O.n_dels.data();
    for (int sd = 0; sd < 2; sd++) {
        LfqIndelColsOwned::Side &S = O.side[sd];
        S.key_chars.push_back('\0');
        lfq_indel_side &T = C.side[sd];
        T.non_fw = S.non_fw.data(); T.non_rv = S.non_rv.data(); T.ne_off = S.ne_off.data();
        T.ne_q = S.ne_q.empty() && S.ne_off.back() > 0 ? nullptr : S.ne_q.data();       /* device-only: lfq_set_indel_arrays_on_host */
        T.ne_mq = S.ne_mq.empty() && S.ne_off.back() > 0 ? nullptr : S.ne_mq.data();
        T.ev_off = S.ev_off.data(); T.key_off = S.key_off.data(); T.key_chars = S.key_chars.data();
        T.ev_fw = S.ev_fw.data(); T.ev_rv = S.ev_rv.data(); T.rd_off = S.rd_off.data();
        T.rd_q = S.rd_q.data(); T.rd_aq = S.rd_aq.data(); T.rd_mq = S.rd_mq.data(); T.rd_sq = S.rd_sq.data();
    }
}

#endif
