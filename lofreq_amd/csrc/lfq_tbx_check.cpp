/*
 * lfq_tbx_check.cpp -- lfq_tbx.h on the host, as a stand-alone program (tests/test_tbi_edges.py compiles it with the host compiler,
 * plainly and sanitized; not part of the library).  One row per line of standard input, one answer per line of standard output; texts
 * and names are hex, "-" stands for none, tables are comma-separated numbers:
 *
 *   build <text> <data_off> <comp_off> <file_off> <name:beg:end,name:beg:end.. or ->
 *       ->   {"error":-1}                           an argument is refused
 *       ->   {"why":w,"line":l}                     the open in tabix mode, or the index (why 8), refuses the file
 *       ->   {"names":["<hex>",..],"conf":[six],"index":{..as lfq_bamidx_check prints a .bai..},"queries":[[[beg,end],..],..]}
 *   parse <tbi>
 *       ->   {"ok":0}  or  {"ok":1,"names":..,"conf":..,"index":..,"bytes":"<hex of the file serialised again>"}
 *
 * The index is built as lfq_vcf_index_build builds it, with loops in place of the kernels (lfq_vc_host_open, lfq_tbx_host_build); the
 * answer printed is that of the .tbi serialised and parsed again, and the program ends with status 3 if the two differ.  The text lives
 * in a vector padded as the device buffer is, the tables in vectors of exactly their length: a read beside them is the sanitizer's.
 */
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lfq_tbx.h"

static bool unhex(const std::string &hex, std::vector<uint8_t> *out)
{
    out->clear();
    for (size_t i = 0; hex != "-" && i + 1 < hex.size(); i += 2) {
        const char b[3] = {hex[i], hex[i + 1], 0};
        char *end = nullptr;
        out->push_back((uint8_t)strtoul(b, &end, 16));
        if (end != b + 2) {
            return false;
        }
    }
    return true;
}

static std::string hex_of(const uint8_t *p, size_t n)
{
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) {
        s.push_back(d[p[i] >> 4]);
        s.push_back(d[p[i] & 15]);
    }
    return s;
}

static std::vector<int64_t> numbers(const std::string &s)
{
    std::vector<int64_t> out;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, ',')) {
        out.push_back(strtoll(item.c_str(), nullptr, 10));
    }
    return out;
}

static bool same(const lfq_vcf_index &a, const lfq_vcf_index &b)
{
    if (a.names != b.names || memcmp(a.conf, b.conf, sizeof(a.conf)) != 0 || a.body.refs.size() != b.body.refs.size()
        || a.body.n_no_coor != b.body.n_no_coor) {
        return false;
    }
    for (size_t t = 0; t < a.body.refs.size(); t++) {
        const LfqBaiRef &x = a.body.refs[t], &y = b.body.refs[t];
        if (x.bins != y.bins || x.linear != y.linear || x.has_meta != y.has_meta
            || (x.has_meta && memcmp(x.meta, y.meta, sizeof(x.meta)) != 0)) {
            return false;
        }
    }
    return true;
}

static void print_index(const lfq_vcf_index &idx)
{
    printf("\"names\":[");
    for (size_t i = 0; i < idx.names.size(); i++) {
        printf("%s\"%s\"", i ? "," : "", hex_of((const uint8_t *)idx.names[i].data(), idx.names[i].size()).c_str());
    }
    printf("],\"conf\":[%d,%d,%d,%d,%d,%d],", idx.conf[0], idx.conf[1], idx.conf[2], idx.conf[3], idx.conf[4], idx.conf[5]);
    printf("\"index\":{\"n_ref\":%zu,\"n_no_coor\":%llu,\"refs\":[", idx.body.refs.size(), (unsigned long long)idx.body.n_no_coor);
    for (size_t t = 0; t < idx.body.refs.size(); t++) {
        const LfqBaiRef &ref = idx.body.refs[t];
        printf("%s{\"bins\":{", t ? "," : "");
        bool first = true;
        for (const auto &kv : ref.bins) {
            printf("%s\"%u\":[", first ? "" : ",", kv.first);
            first = false;
            for (size_t k = 0; k < kv.second.size(); k++) {
                printf("%s[%llu,%llu]", k ? "," : "", (unsigned long long)kv.second[k].first, (unsigned long long)kv.second[k].second);
            }
            printf("]");
        }
        printf("},\"linear\":[");
        for (size_t w = 0; w < ref.linear.size(); w++) {
            printf("%s%llu", w ? "," : "", (unsigned long long)ref.linear[w]);
        }
        if (ref.has_meta) {
            printf("],\"meta\":[[%llu,%llu],[%llu,%llu]]}", (unsigned long long)ref.meta[0], (unsigned long long)ref.meta[1],
                   (unsigned long long)ref.meta[2], (unsigned long long)ref.meta[3]);
        } else {
            printf("],\"meta\":null}");
        }
    }
    printf("]}");
}

static int do_build(std::stringstream &ss)
{
    std::string f[5];
    ss >> f[0] >> f[1] >> f[2] >> f[3] >> f[4];
    std::vector<uint8_t> text;
    if (!ss || !unhex(f[0], &text)) {
        return 2;
    }
    const std::vector<int64_t> data_off = numbers(f[1]), comp_off = numbers(f[2]);
    const int64_t file_off = strtoll(f[3].c_str(), nullptr, 10), n_blocks = (int64_t)data_off.size() - 1;
    if (n_blocks < 0 || comp_off.size() != data_off.size()
        || !lfq_tbx_check_args((int64_t)text.size(), data_off.data(), comp_off.data(), n_blocks, file_off)) {
        printf("{\"error\":-1}\n");
        return 0;
    }
    const int64_t n_kept = lfq_tbx_trim_blocks(data_off.data(), n_blocks);
    LfqVcHostFile F;
    int64_t bad_line = 0;
    int why = lfq_vc_host_open(text.data(), (int64_t)text.size(), LFQ_VC_TABIX, &F, &bad_line);
    lfq_vcf_index idx, back;
    if (why == LFQ_VC_OK) {
        why = lfq_tbx_host_build(F, data_off.data(), comp_off.data(), n_kept, file_off, &idx, &bad_line);
        if (why < 0) {
            return 4;
        }
    }
    if (why != LFQ_VC_OK) {
        printf("{\"why\":%d,\"line\":%lld}\n", why, (long long)bad_line);
        return 0;
    }
    lfq_tbx_serialise(idx, &idx.bytes);
    if (!lfq_tbx_parse(idx.bytes.data(), (int64_t)idx.bytes.size(), &back) || !same(idx, back)) {
        return 3;
    }
    printf("{");
    print_index(back);
    printf(",\"queries\":[");
    std::stringstream qs(f[4] == "-" ? "" : f[4]);
    std::string q;
    bool first = true;
    while (std::getline(qs, q, ',')) {
        const size_t a = q.find(':'), b = q.find(':', a + 1);
        std::vector<uint8_t> name;
        if (a == std::string::npos || b == std::string::npos || !unhex(q.substr(0, a), &name)) {
            return 2;
        }
        const std::string chrom((const char *)name.data(), name.size());
        lfq_tbx_query(&back, chrom.c_str(), strtoll(q.c_str() + a + 1, nullptr, 10), strtoll(q.c_str() + b + 1, nullptr, 10));
        printf("%s[", first ? "" : ",");
        first = false;
        for (size_t k = 0; k < back.body.q_beg.size(); k++) {
            printf("%s[%llu,%llu]", k ? "," : "", (unsigned long long)back.body.q_beg[k], (unsigned long long)back.body.q_end[k]);
        }
        printf("]");
    }
    printf("]}\n");
    return 0;
}

static int do_parse(std::stringstream &ss)
{
    std::string hex;
    ss >> hex;
    std::vector<uint8_t> tbi;
    if (!ss || !unhex(hex, &tbi)) {
        return 2;
    }
    lfq_vcf_index idx;
    const std::vector<uint8_t> exact(tbi.begin(), tbi.end());         /* (exactly the file: no slack behind it) */
    if (!lfq_tbx_parse(exact.data(), (int64_t)exact.size(), &idx)) {
        printf("{\"ok\":0}\n");
        return 0;
    }
    lfq_tbx_serialise(idx, &idx.bytes);
    printf("{\"ok\":1,");
    print_index(idx);
    printf(",\"bytes\":\"%s\"}\n", hex_of(idx.bytes.data(), idx.bytes.size()).c_str());
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') {
            continue;
        }
        std::stringstream ss(line);
        std::string what;
        ss >> what;
        const int rc = what == "build" ? do_build(ss) : what == "parse" ? do_parse(ss) : 2;
        if (rc != 0) {
            return rc;
        }
    }
    return 0;
}
