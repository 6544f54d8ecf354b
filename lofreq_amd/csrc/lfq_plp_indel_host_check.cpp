/*
 * lfq_plp_indel_host_check.cpp -- lfq_plp_indel_host.h on the host, as a stand-alone program (tests/test_plp_indel_host.py compiles
 * it with the host compiler; not part of the library).  It runs the stages in the order lfq_readset_pileup_indels does, serially
 * and part by part with the numbers of parts the input forces; the kernel's nine per-position counters are input, the gather of
 * ai / ad on the device is an indexed read here.
 *
 * Input, any number of cases, whitespace-separated integers but for the reference:
 *   n ref_len begin end min_plp_idq  scan_parts table_parts col_parts  all_columns have_qsum gather  idq_mode idq_ins idq_del
 *   has_bi has_bd has_ai has_ad has_sq has_keep                        (0: that array is a null pointer)
 *   ref                                                                (ref_len letters; "-" for none)
 *   per read:  pos mapq reverse flags sq keep n_cigar l_seq   cigar[n_cigar] (len << 4 | op)   seq[l_seq]  bi[] bd[] ai[] ad[]
 *   9 x (end - begin) counters; without have_qsum: per side the number of non-event qualities and the qualities (ne_q)
 * Output per case:
 *   N <columns> <ne_total 0> <ne_total 1> <events>
 *   C <pos> <ref> cov tails non_indels n_ins n_dels hrun cons   and per side  non_fw non_rv ne_off[col] ne_off[col + 1] qsum
 *   E <pos> <side> <key> fw rv : rd_q : rd_aq : rd_mq : rd_sq          per event, in table order
 *   P <pos> <column or -1> <pos_off 0> <pos_off 1>                     per position of the region
 *   END
 */
#include <stdio.h>
#include <stdlib.h>

#include "lfq_plp_indel_host.h"

/* the Dindel byte of a base is lfq_indelqual.hip's business (tests/test_gpu_indelqual.py); a stand-in that depends on all it is given */
uint8_t lfq_idq_host_byte(const char *ref, int64_t ref_len, int64_t pos, const uint32_t *cigar, int n_cigar, int64_t qpos)
{
    return (uint8_t)(33 + (pos + qpos + n_cigar + (int64_t)(cigar[0] >> 4) + (ref_len > 0 ? ref[0] : 0)) % 40);
}

static bool get(long long *v)
{
    return scanf("%lld", v) == 1;
}

template <typename T>
static bool get_n(std::vector<T> &v, long long n)
{
    for (long long i = 0, x; i < n; i++) {
        if (!get(&x)) {
            return false;
        }
        v.push_back((T)x);
    }
    return true;
}

static void print_list(const int16_t *v, int64_t a, int64_t b)
{
    printf(" :");
    for (int64_t i = a; i < b; i++) {
        printf(" %d", (int)v[i]);
    }
}

int main(void)
{
    long long hd[20];
    while (get(&hd[0])) {
        for (int i = 1; i < 20; i++) {
            if (!get(&hd[i])) {
                return 2;
            }
        }
        const int64_t n = hd[0], ref_len = hd[1], begin = hd[2], end = hd[3], width = end - begin;
        const int min_idq = (int)hd[4], scan_parts = (int)hd[5], table_parts = (int)hd[6], col_parts = (int)hd[7];
        const bool all_columns = hd[8] != 0, have_qsum = hd[9] != 0, gather = hd[10] != 0;
        char word[4096];
        if (n < 0 || width < 0 || ref_len < 0 || ref_len >= (int64_t)sizeof(word) || scan_parts < 1 || table_parts < 1
            || col_parts < 1 || scanf("%4095s", word) != 1 || (ref_len > 0 && (int64_t)strlen(word) != ref_len)) {
            return 2;
        }
        const std::string ref(ref_len > 0 ? word : "");
        std::vector<int32_t> pos, sq;
        std::vector<int64_t> cigar_off(1, 0), seq_off(1, 0);
        std::vector<uint32_t> cigar;
        std::vector<uint8_t> mapq, reverse, fl, keep, seq, tag[4];
        for (int64_t r = 0; r < n; r++) {
            long long v[8];
            for (int i = 0; i < 8; i++) {
                if (!get(&v[i])) {
                    return 2;
                }
            }
            pos.push_back((int32_t)v[0]);
            mapq.push_back((uint8_t)v[1]);
            reverse.push_back((uint8_t)v[2]);
            fl.push_back((uint8_t)v[3]);
            sq.push_back((int32_t)v[4]);
            keep.push_back((uint8_t)v[5]);
            if (v[6] < 1 || v[7] < 0 || !get_n(cigar, v[6]) || !get_n(seq, v[7]) || !get_n(tag[0], v[7]) || !get_n(tag[1], v[7])
                || !get_n(tag[2], v[7]) || !get_n(tag[3], v[7])) {
                return 2;
            }
            cigar_off.push_back((int64_t)cigar.size());
            seq_off.push_back((int64_t)seq.size());
        }
        std::vector<int32_t> cnt[9];
        const int32_t *h[9];
        for (int i = 0; i < 9; i++) {
            if (!get_n(cnt[i], width)) {
                return 2;
            }
            h[i] = cnt[i].data();
        }
        LfqPlpReads R = {};
        R.pos = pos.data(); R.cigar_off = cigar_off.data(); R.seq_off = seq_off.data(); R.cigar = cigar.data();
        R.seq = seq.data(); R.mapq = mapq.data(); R.reverse = reverse.data(); R.ref = ref.c_str(); R.ref_len = ref_len;
        R.bi = hd[14] ? tag[0].data() : nullptr; R.bd = hd[15] ? tag[1].data() : nullptr;
        R.ai = hd[16] ? tag[2].data() : nullptr; R.ad = hd[17] ? tag[3].data() : nullptr;
        R.fl = fl.data(); R.sq = hd[18] ? sq.data() : nullptr; R.keep = hd[19] ? keep.data() : nullptr;
        R.idq_mode = (int)hd[11]; R.idq_ins = (uint8_t)hd[12]; R.idq_del = (uint8_t)hd[13];

        LfqIndelColsOwned O;
        memset(&O.cols, 0, sizeof(O.cols));
        /* 1. events */
        std::vector<LfqPlpEv> evs;
        std::vector<std::vector<LfqPlpEv>> evs_part((size_t)scan_parts);
        for (int p = 0; p < scan_parts; p++) {
            lfq_plp_scan_events(R, n * p / scan_parts, n * (p + 1) / scan_parts, begin, end, min_idq, evs_part[(size_t)p]);
        }
        lfq_plp_merge_events(evs_part.data(), scan_parts, evs);
        /* 4a. tables */
        const std::vector<size_t> cut = lfq_plp_table_cuts(evs, table_parts);
        std::vector<LfqPlpPartTables> pt((size_t)table_parts);
        for (int t = 0; t < table_parts; t++) {
            lfq_plp_build_tables(R, evs, cut[(size_t)t], cut[(size_t)t + 1], begin, pt[(size_t)t]);
        }
        LfqPlpTables T;
        lfq_plp_append_tables(pt, O, T);
        /* 3. columns */
        std::vector<int64_t> off[2] = {std::vector<int64_t>((size_t)width, -7), std::vector<int64_t>((size_t)width, -7)};
        int64_t *const pos_off[2] = {off[0].data(), off[1].data()};
        std::vector<int32_t> col_of((size_t)width, -7);
        std::vector<int64_t> col_pos((size_t)width, -7);
        std::vector<uint8_t> has_ev;
        lfq_plp_mark_events(evs, begin, width, all_columns, has_ev);
        std::vector<LfqPlpPartCount> pc((size_t)col_parts + 1, LfqPlpPartCount{0, {0, 0}});
        for (int p = 0; p < col_parts; p++) {
            pc[(size_t)p + 1] = lfq_plp_cols_count(h, has_ev, width * p / col_parts, width * (p + 1) / col_parts);
        }
        lfq_plp_cols_alloc(O, pc.data(), col_parts, have_qsum);
        for (int p = 0; p < col_parts; p++) {
            lfq_plp_cols_fill(R, h, has_ev, begin, width * p / col_parts, width * (p + 1) / col_parts, pc[(size_t)p], have_qsum, O,
                              col_of.data(), pos_off, col_pos.data());
        }
        const int64_t ne_total[2] = {pc[(size_t)col_parts].ne[0], pc[(size_t)col_parts].ne[1]};
        if (!have_qsum) {                       /* what the scatter pass brings back */
            for (int sd = 0; sd < 2; sd++) {
                long long m = 0;
                std::vector<int16_t> q;
                if (!get(&m) || m != ne_total[sd] || !get_n(q, m)) {
                    return 3;
                }
                O.side[sd].ne_q.assign(q.begin(), q.end());
                O.side[sd].ne_mq.assign(q.size(), 0);
            }
        }
        /* the gather, 4. ev_off, 5. consensus, 4b. rd_aq, 6. publish */
        std::vector<int64_t> idx(evs.size());
        std::vector<uint8_t> g(2 * evs.size());
        lfq_plp_gather_index(R, evs, idx.data());
        for (size_t i = 0; i < evs.size() && gather; i++) {
            g[i] = tag[2][(size_t)idx[i]];
            g[evs.size() + i] = tag[3][(size_t)idx[i]];
        }
        if (!lfq_plp_fill_ev_off(T, col_of.data(), O)) {
            return 4;
        }
        lfq_plp_cons_flags(T, col_of.data(), have_qsum, O);
        lfq_plp_fill_rd_aq(R, evs, T, gather ? g.data() : nullptr, gather ? g.data() + evs.size() : nullptr, O);
        lfq_plp_publish(O);

        const lfq_indel_columns &C = O.cols;
        printf("N %lld %lld %lld %zu\n", (long long)C.ncols, (long long)ne_total[0], (long long)ne_total[1], evs.size());
        for (int64_t col = 0; col < C.ncols; col++) {
            printf("C %lld %c %d %d %d %d %d %d %d", (long long)col_pos[(size_t)col], (char)C.ref_base[col], C.coverage_plp[col],
                   C.num_tails[col], C.num_non_indels[col], C.num_ins[col], C.num_dels[col], C.hrun[col], (int)C.cons_indel[col]);
            for (int sd = 0; sd < 2; sd++) {
                const lfq_indel_side &S = C.side[sd];
                printf("  %d %d %lld %lld %d", S.non_fw[col], S.non_rv[col], (long long)S.ne_off[col], (long long)S.ne_off[col + 1],
                       have_qsum ? O.ne_qsum[sd][(size_t)col] : -1);
            }
            printf("\n");
            for (int sd = 0; sd < 2; sd++) {
                const lfq_indel_side &S = C.side[sd];
                for (int64_t e = S.ev_off[col]; e < S.ev_off[col + 1]; e++) {
                    printf("E %lld %d %.*s %d %d", (long long)col_pos[(size_t)col], sd, (int)(S.key_off[e + 1] - S.key_off[e]),
                           S.key_chars + S.key_off[e], S.ev_fw[e], S.ev_rv[e]);
                    print_list(S.rd_q, S.rd_off[e], S.rd_off[e + 1]);
                    print_list(S.rd_aq, S.rd_off[e], S.rd_off[e + 1]);
                    print_list(S.rd_mq, S.rd_off[e], S.rd_off[e + 1]);
                    print_list(S.rd_sq, S.rd_off[e], S.rd_off[e + 1]);
                    printf("\n");
                }
            }
        }
        for (int64_t p = 0; p < width; p++) {
            printf("P %lld %d %lld %lld\n", (long long)(begin + p), col_of[(size_t)p], (long long)off[0][(size_t)p], (long long)off[1][(size_t)p]);
        }
        printf("END\n");
    }
    return 0;
}
