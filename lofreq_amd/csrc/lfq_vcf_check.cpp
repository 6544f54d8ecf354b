/*
 * lfq_vcf_check.cpp -- lfq_vcf.h on the host, as a stand-alone program (tests/test_vcf_edges.py compiles it with the host compiler,
 * plainly and sanitized; not part of the library).  One row per line of standard input, one answer per line of standard output; every
 * text is hex, "-" stands for none:
 *
 *   open <mode> <text>
 *       ->   {"why":w,"line":l}                                                   the file is refused
 *       ->   {"n_rec":..,"behind":..,"found":0|1,"header":"<hex>","recs":[[line,pos,qual,flags,nf,[off x 10]],..],
 *             "runs":[["<hex name>",first record],..],"info":[[dp,sb,fw,rv,"<hex of AF's value>"|null],..]}
 *   set <op> <only_passed> <only_pos> <only_snvs> <only_indels> <count_only> <add> <text 1> <text 2> [<more texts>]
 *       ->   {"why":w,"file":f,"line":l}  or  {"counts":[n_vars1,n_ignored,n_out],"keep":[..],"text":"<hex>"}
 *       ->   {"open":[file,why,line]}                                             one of the files is refused when opened
 *   mask <text> <chrom> <ref_len> <bed: beg:end,beg:end or ->
 *       ->   {"mask":[positions set]}
 *
 * The texts live in vectors padded as the device buffer is (lfq_vc_host_open), so a read beside them is the sanitizer's to find.
 */
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lfq_vcf.h"

static int hexval(char ch)
{
    return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
}

static bool unhex(const std::string &hex, std::vector<uint8_t> *out)
{
    out->clear();
    for (size_t i = 0; hex != "-" && i + 1 < hex.size(); i += 2) {
        const int hi = hexval(hex[i]), lo = hexval(hex[i + 1]);
        if (hi < 0 || lo < 0) {
            return false;
        }
        out->push_back((uint8_t)(hi * 16 + lo));
    }
    return true;
}

static void put_hex(const uint8_t *p, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        printf("%02x", p[i]);
    }
}

static int do_open(std::stringstream &ss)
{
    int mode = 0;
    std::string hex;
    std::vector<uint8_t> text;
    if (!(ss >> mode >> hex) || !unhex(hex, &text)) {
        return 2;
    }
    LfqVcHostFile F;
    int64_t bad_line = 0;
    const int why = lfq_vc_host_open(text.data(), (int64_t)text.size(), mode, &F, &bad_line);
    if (why != LFQ_VC_OK) {
        printf("{\"why\":%d,\"line\":%lld}\n", why, (long long)bad_line);
        return 0;
    }
    const LfqVcTab T = F.tab();
    const int64_t hdr = F.hdr_line >= 0 ? std::min(F.lstart[(size_t)F.hdr_line + 1], F.n) : 0;
    printf("{\"n_rec\":%lld,\"behind\":%lld,\"found\":%d,\"header\":\"", (long long)F.n_rec, (long long)F.lines_behind, F.hdr_line >= 0 ? 1 : 0);
    put_hex(F.text.data(), (size_t)hdr);
    printf("\",\"recs\":[");
    for (int64_t r = 0; r < F.n_rec; r++) {
        const int64_t k = lfq_vc_line_of(T, r);
        printf("%s[%lld,%lld,%d,%d,%d,[", r ? "," : "", (long long)k, (long long)F.pos[(size_t)k], F.qual[(size_t)k],
               F.flags[(size_t)k] & 31, F.nf[(size_t)k]);
        for (int j = 0; j < LFQ_VC_NOFF; j++) {
            printf("%s%d", j ? "," : "", F.off[(size_t)k * LFQ_VC_NOFF + j]);
        }
        printf("]]");
    }
    printf("],\"runs\":[");
    for (size_t i = 0; i < F.run_name.size(); i++) {
        printf("%s[\"", i ? "," : "");
        put_hex((const uint8_t *)F.run_name[i].data(), F.run_name[i].size());
        printf("\",%lld]", (long long)F.run_beg[i]);
    }
    printf("],\"info\":[");
    for (int64_t r = 0; r < F.n_rec; r++) {
        LfqVcInfo I;
        lfq_vc_info_values(T, lfq_vc_line_of(T, r), &I);
        printf("%s[%d,%d,%d,%d,", r ? "," : "", I.dp, I.sb, I.dp4[2], I.dp4[3]);
        if (I.has & 8) {
            printf("\"");
            put_hex(F.text.data() + I.af_beg, (size_t)I.af_len);
            printf("\"]");
        } else {
            printf("null]");
        }
    }
    printf("]}\n");
    return 0;
}

static int do_set(std::stringstream &ss)
{
    LfqVcSetConf c;
    int count_only = 0;
    std::string add_hex, hex;
    std::vector<uint8_t> add;
    if (!(ss >> c.op >> c.only_passed >> c.only_pos >> c.only_snvs >> c.only_indels >> count_only >> add_hex) || !unhex(add_hex, &add)) {
        return 2;
    }
    std::vector<LfqVcHostFile> files;
    std::vector<std::vector<uint8_t>> texts;
    while (ss >> hex) {
        texts.emplace_back();
        if (!unhex(hex, &texts.back())) {
            return 2;
        }
    }
    if (texts.size() < 2) {
        return 2;
    }
    files.resize(texts.size());
    for (size_t i = 0; i < texts.size(); i++) {
        if (i == 1 && c.op == LFQ_VC_OP_CONCAT) {
            continue;                   /* "-": concat has no file 2 */
        }
        int64_t bad_line = 0;
        const int why = lfq_vc_host_open(texts[i].data(), (int64_t)texts[i].size(), i == 1 ? LFQ_VC_TABIX : LFQ_VC_STREAM, &files[i], &bad_line);
        if (why != LFQ_VC_OK) {
            printf("{\"open\":[%d,%d,%lld]}\n", (int)i, why, (long long)bad_line);
            return 0;
        }
    }
    std::vector<const LfqVcHostFile *> ones(1, &files[0]);
    for (size_t i = 2; i < files.size(); i++) {
        ones.push_back(&files[i]);
    }
    LfqVcSetOut out;
    lfq_vc_host_set(ones, &files[1], c, std::string(add.begin(), add.end()), count_only != 0, &out);
    if (out.why != LFQ_VC_OK) {
        printf("{\"why\":%d,\"file\":%d,\"line\":%lld}\n", out.why, out.bad_file, (long long)out.bad_line);
        return 0;
    }
    printf("{\"counts\":[%lld,%lld,%lld],\"keep\":[", (long long)out.n_vars1, (long long)out.n_ignored, (long long)out.n_out);
    for (size_t i = 0; i < out.keep.size(); i++) {
        printf("%s%d", i ? "," : "", out.keep[i]);
    }
    printf("],\"text\":\"");
    put_hex((const uint8_t *)out.text.data(), out.text.size());
    printf("\"}\n");
    return 0;
}

static int do_mask(std::stringstream &ss)
{
    std::string hex, chrom_hex, bed_s;
    long long ref_len = 0;
    std::vector<uint8_t> text, chrom;
    if (!(ss >> hex >> chrom_hex >> ref_len >> bed_s) || !unhex(hex, &text) || !unhex(chrom_hex, &chrom)) {
        return 2;
    }
    LfqVcHostFile F;
    int64_t bad_line = 0;
    if (lfq_vc_host_open(text.data(), (int64_t)text.size(), LFQ_VC_STREAM, &F, &bad_line) != LFQ_VC_OK) {
        return 2;
    }
    std::vector<std::pair<int32_t, int32_t>> iv;
    if (bed_s != "-") {
        std::stringstream bs(bed_s);
        std::string one;
        while (std::getline(bs, one, ',')) {
            const size_t colon = one.find(':');
            iv.emplace_back((int32_t)atol(one.c_str()), (int32_t)atol(one.c_str() + colon + 1));
        }
        std::sort(iv.begin(), iv.end());
    }
    std::vector<int32_t> beg, pmax;
    for (const auto &x : iv) {
        beg.push_back(x.first);
        pmax.push_back(pmax.empty() ? x.second : std::max(pmax.back(), x.second));
    }
    const LfqBedTab tab = {beg.data(), pmax.data(), bed_s == "-" ? -1 : (int64_t)beg.size()};
    const LfqVcTab T = F.tab();
    std::vector<uint8_t> mask((size_t)ref_len, 0);
    const std::string name(chrom.begin(), chrom.end());
    for (int64_t r = 0; r < F.n_rec; r++) {
        const int64_t p = F.pos[(size_t)lfq_vc_line_of(T, r)];
        if (F.run_name[(size_t)F.run_id[(size_t)r]] == name && lfq_vc_mask_hit(p, ref_len, tab)) {
            mask[(size_t)p] = 1;
        }
    }
    printf("{\"mask\":[");
    bool first = true;
    for (long long i = 0; i < ref_len; i++) {
        if (mask[(size_t)i]) {
            printf("%s%lld", first ? "" : ",", i);
            first = false;
        }
    }
    printf("]}\n");
    return 0;
}

int main()
{
    std::string row;
    while (std::getline(std::cin, row)) {
        std::stringstream ss(row);
        std::string what;
        ss >> what;
        const int rc = what == "open" ? do_open(ss) : what == "set" ? do_set(ss) : what == "mask" ? do_mask(ss) : 2;
        if (rc != 0) {
            fprintf(stderr, "bad row\n");
            return rc;
        }
    }
    return 0;
}
