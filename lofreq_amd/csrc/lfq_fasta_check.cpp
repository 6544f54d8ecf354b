/*
 * lfq_fasta_check.cpp -- lfq_fasta.h on the host, as a stand-alone program (tests/test_fasta_edges.py compiles it with the host
 * compiler, plainly and sanitized; not part of the library).  One row per line of standard input, one answer per line of standard
 * output:
 *
 *   <hex of the FASTA bytes, or -> <hex of a .fai text to fetch by, or ->
 *       ->   {"fai":"<hex>","n_dup":k,"fetch":["<hex>"|null,...],"masks":1}   the index (built, or the parsed one) and every contig of it
 *       ->   {"error":[why,line,byte],"masks":1}                               the file is refused
 *       ->   {"parse_error":1}                                                 the .fai text is refused
 *
 * "masks": the chunk masks of the kernels (lfq_fa_chunk_masks, lfq_fa_line_starts), run over the bytes 16 at a time, give the graph
 * count and the line starts a byte loop gives; the program exits with status 3 where they do not.  `--time N` instead of rows: the
 * one-thread index build of an N-byte synthetic contig at width 60, milliseconds on standard output.
 * The bytes live in a vector of exactly their length, so a read beside them is the sanitizer's to find.
 */
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lfq_fasta.h"

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

static void put_hex(const std::string &s)
{
    for (unsigned char ch : s) {
        printf("%02x", ch);
    }
}

/* the kernels' view of the bytes: chunks of 16 from a zero-padded copy */
static bool masks_agree(const std::vector<uint8_t> &text)
{
    const int64_t n = (int64_t)text.size(), n_chunks = (n + LFQ_FA_CHUNK - 1) / LFQ_FA_CHUNK;
    std::vector<uint8_t> pad((size_t)n_chunks * LFQ_FA_CHUNK + 16, 0);
    std::copy(text.begin(), text.end(), pad.begin());
    std::vector<int64_t> want, got;
    lfq_fa_host_lines(text.data(), n, &want);
    int64_t graph = 0, graph_want = 0, headers = 0, headers_want = 0;
    if (n > 0) {
        got.push_back(0);
    }
    for (int64_t c = 0; c < n_chunks; c++) {
        uint32_t w[4];
        memcpy(w, pad.data() + c * LFQ_FA_CHUNK, 16);
        const LfqFaMasks m = lfq_fa_chunk_masks(w[0], w[1], w[2], w[3]);
        graph += __builtin_popcount(m.graph);
        const uint32_t prev = c == 0 ? 1u : (uint32_t)(pad[(size_t)(c * LFQ_FA_CHUNK - 1)] == '\n');
        headers += __builtin_popcount(((m.nl << 1) | prev) & m.gt & 0xffffu);
        for (uint32_t s = lfq_fa_line_starts(m.nl, c, n); s; s &= s - 1) {
            got.push_back(c * LFQ_FA_CHUNK + __builtin_ctz(s) + 1);
        }
    }
    if (n > 0) {
        got.push_back(text[(size_t)n - 1] == '\n' ? n : n + 1);
    }
    for (int64_t i = 0; i < n; i++) {
        graph_want += lfq_fa_isgraph(text[(size_t)i]);
        headers_want += text[(size_t)i] == '>' && (i == 0 || text[(size_t)i - 1] == '\n');
    }
    return got == want && graph == graph_want && headers == headers_want;
}

static int time_build(int64_t n)
{
    std::vector<uint8_t> text;
    text.reserve((size_t)n + 64);
    const char *head = ">big\n";
    text.insert(text.end(), head, head + 5);
    for (int64_t i = 0; (int64_t)text.size() < n; i++) {
        text.push_back((uint8_t)"ACGT"[(i * 2654435761u >> 7) & 3]);
        if (i % 60 == 59) {
            text.push_back('\n');
        }
    }
    text.push_back('\n');
    lfq_fasta_index idx;
    int why = 0, bad_byte = 0;
    int64_t bad_line = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = lfq_fa_host_build(text.data(), (int64_t)text.size(), &idx, &why, &bad_line, &bad_byte);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    printf("{\"n_bytes\":%lld,\"ok\":%d,\"length\":%lld,\"build_ms\":%.3f}\n", (long long)text.size(), ok ? 1 : 0,
           ok ? (long long)idx.e[0].length : 0ll, ms);
    return ok ? 0 : 3;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "--time") {
        return time_build(strtoll(argv[2], nullptr, 10));
    }
    std::string row;
    while (std::getline(std::cin, row)) {
        std::stringstream ss(row);
        std::string hex, fai_hex;
        std::vector<uint8_t> text, fai;
        if (!(ss >> hex >> fai_hex) || !unhex(hex, &text) || !unhex(fai_hex, &fai)) {
            fprintf(stderr, "bad row\n");
            return 2;
        }
        if (!masks_agree(text)) {
            fprintf(stderr, "the chunk masks disagree with the byte loop\n");
            return 3;
        }
        lfq_fasta_index idx;
        if (fai_hex != "-") {
            if (!lfq_fa_index_parse_text((const char *)fai.data(), (int64_t)fai.size(), &idx)) {
                printf("{\"parse_error\":1}\n");
                continue;
            }
        } else {
            int why = 0, bad_byte = 0;
            int64_t bad_line = 0;
            if (!lfq_fa_host_build(text.data(), (int64_t)text.size(), &idx, &why, &bad_line, &bad_byte)) {
                printf("{\"error\":[%d,%lld,%d],\"masks\":1}\n", why, (long long)bad_line, bad_byte);
                continue;
            }
        }
        printf("{\"fai\":\"");
        put_hex(lfq_fa_index_text(&idx));
        printf("\",\"n_dup\":%lld,\"fetch\":[", (long long)idx.n_dup);
        for (size_t i = 0; i < idx.e.size(); i++) {
            std::string seq;
            printf("%s", i ? "," : "");
            if (lfq_fa_host_fetch(text.data(), (int64_t)text.size(), idx.e[i], &seq)) {
                printf("\"");
                put_hex(seq);
                printf("\"");
            } else {
                printf("null");
            }
        }
        printf("],\"masks\":1}\n");
    }
    return 0;
}
