/*
 * lfq_bamidx_check.cpp -- lfq_bamidx.h on the host, as a stand-alone program (tests/test_bai_edges.py compiles it with the host
 * compiler, plainly and sanitized; not part of the library).  One row per line of standard input, one answer per line of standard
 * output:
 *
 *   <hex of the body> <rec_off> <data_off> <comp_off> <file_off> <n_ref>   ->   the parsed index as JSON, or {"error":<record>}
 *
 * the three offset tables as comma-separated numbers; record -1: an argument is refused.  The index is built as
 * lfq_bam_index_build builds it, with loops in place of the kernels: the record pass over every record (the smallest refused index
 * wins), lfq_bai_compact_host for the chunks, runs and intervals, lfq_bai_finish.  The body vector holds exactly the body, so a read
 * beside it is the sanitizer's to find; the answer printed is that of the .bai serialised and parsed again, and the program ends
 * with status 3 if the two differ.
 *
 *   lfq_bamidx_check --time <file> <passes>     (profiles/bai_rate.py)
 *
 * reads one row from a binary file -- int64 n_bytes, n_recs, n_blocks, file_off, n_ref, then rec_off, data_off, comp_off and the
 * body -- and prints the milliseconds of each pass of the same build on one thread, then the index.
 */
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lfq_bamidx.h"

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

static bool same(const lfq_bam_index &a, const lfq_bam_index &b)
{
    if (a.refs.size() != b.refs.size() || a.n_no_coor != b.n_no_coor) {
        return false;
    }
    for (size_t t = 0; t < a.refs.size(); t++) {
        const LfqBaiRef &x = a.refs[t], &y = b.refs[t];
        if (x.bins != y.bins || x.linear != y.linear || x.has_meta != y.has_meta
            || (x.has_meta && memcmp(x.meta, y.meta, sizeof(x.meta)) != 0)) {
            return false;
        }
    }
    return true;
}

static void print(const lfq_bam_index &idx)
{
    printf("{\"n_ref\":%zu,\"n_no_coor\":%llu,\"refs\":[", idx.refs.size(), (unsigned long long)idx.n_no_coor);
    for (size_t t = 0; t < idx.refs.size(); t++) {
        const LfqBaiRef &ref = idx.refs[t];
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
    printf("]}\n");
}

/* one build as lfq_bam_index_build makes it; -> the refused record, -1 an argument, -2 none */
static int64_t build(const std::vector<uint8_t> &body, const std::vector<int64_t> &rec_off, const std::vector<int64_t> &data_off,
                     const std::vector<int64_t> &comp_off, int64_t file_off, int32_t n_ref, lfq_bam_index *idx)
{
    const int64_t n_recs = (int64_t)rec_off.size() - 1, n_blocks = (int64_t)data_off.size() - 1;
    if (n_recs < 0 || n_blocks < 0 || comp_off.size() != data_off.size()
        || !lfq_bai_check_args((int64_t)body.size(), rec_off.data(), n_recs, data_off.data(), comp_off.data(), n_blocks, file_off, n_ref)) {
        return -1;
    }
    std::vector<LfqBaiRec> recs((size_t)n_recs);
    int64_t bad = -2;
    for (int64_t j = n_recs - 1; j >= 0; j--) {         /* any order: the smallest refused index is kept */
        if (!lfq_bai_record(body.data(), rec_off.data(), j, n_ref, data_off.data(), comp_off.data(), n_blocks, file_off,
                            &recs[(size_t)j])) {
            bad = j;
        }
    }
    if (bad >= 0) {
        return bad;
    }
    std::vector<LfqBaiChunk> chunks;
    std::vector<LfqBaiRun> runs;
    std::vector<LfqBaiIntv> intvs;
    lfq_bai_compact_host(recs.data(), n_recs, &chunks, &runs, &intvs);
    if (!lfq_bai_finish(chunks.data(), (int64_t)chunks.size(), runs.data(), (int64_t)runs.size(), intvs.data(), (int64_t)intvs.size(),
                        n_ref, n_recs, idx)) {
        exit(4);
    }
    return -2;
}

static int time_file(const char *path, int passes)
{
    FILE *f = fopen(path, "rb");
    int64_t h[5];
    if (!f || fread(h, 8, 5, f) != 5 || h[0] < 0 || h[1] < 0 || h[2] < 0) {
        return 2;
    }
    std::vector<int64_t> rec_off((size_t)h[1] + 1), data_off((size_t)h[2] + 1), comp_off((size_t)h[2] + 1);
    std::vector<uint8_t> body((size_t)h[0]);
    if (fread(rec_off.data(), 8, rec_off.size(), f) != rec_off.size() || fread(data_off.data(), 8, data_off.size(), f) != data_off.size()
        || fread(comp_off.data(), 8, comp_off.size(), f) != comp_off.size() || fread(body.data(), 1, body.size(), f) != body.size()) {
        return 2;
    }
    fclose(f);
    lfq_bam_index idx;
    for (int p = 0; p < passes; p++) {
        idx = lfq_bam_index();
        const auto t0 = std::chrono::steady_clock::now();
        if (build(body, rec_off, data_off, comp_off, h[3], (int32_t)h[4], &idx) != -2) {
            return 5;
        }
        printf("%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    print(idx);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::string(argv[1]) == "--time") {
        return time_file(argv[2], atoi(argv[3]));
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') {
            continue;
        }
        std::stringstream ss(line);
        std::string hex, f[5];
        ss >> hex >> f[0] >> f[1] >> f[2] >> f[3] >> f[4];
        if (!ss) {
            return 2;
        }
        std::vector<uint8_t> body;
        if (hex != "-") {                       /* "-": an empty body */
            for (const char *e = hex.c_str(); e[0] && e[1]; e += 2) {
                const char b[3] = {e[0], e[1], 0};
                body.push_back((uint8_t)strtoul(b, nullptr, 16));
            }
        }
        const std::vector<int64_t> rec_off = numbers(f[0]), data_off = numbers(f[1]), comp_off = numbers(f[2]);
        const int64_t file_off = strtoll(f[3].c_str(), nullptr, 10);
        const int32_t n_ref = (int32_t)strtol(f[4].c_str(), nullptr, 10);
        lfq_bam_index idx, back;
        const int64_t bad = build(body, rec_off, data_off, comp_off, file_off, n_ref, &idx);
        if (bad != -2) {
            printf("{\"error\":%lld}\n", (long long)bad);
            continue;
        }
        lfq_bai_serialise(idx, &idx.bytes);
        if (!lfq_bai_parse(idx.bytes.data(), (int64_t)idx.bytes.size(), &back) || !same(idx, back)) {
            return 3;
        }
        print(back);
    }
    return 0;
}
