/*
 * lfq_inflate_check.cpp -- lfq_inflate.h on the host, as a stand-alone program (tests/test_bgzf_edges.py compiles it with the host
 * compiler; not part of the library).  One raw deflate stream per line of standard input, one answer per line of standard output:
 *
 *   <isize> <hex of the stream, or - for an empty one>   ->   <status> <bytes written> <crc32, hex> <hex of the output, or ->
 *
 * status is LFQ_INF_* of the header; the CRC is that of the bytes written, computed as the device computes it: 64 slices, each
 * multiplied by x^(8 * bytes behind it) modulo the polynomial.  The input vector holds exactly the stream and the output vector
 * exactly isize bytes, and every access goes through vector::at: one beside them ends the program, sanitized or not.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "lfq_inflate.h"

struct HostIo {
    const std::vector<uint8_t> *in;
    std::vector<uint8_t> *out;
    uint32_t in8(int64_t p) { return in->at((size_t)p); }
    uint32_t in32(int64_t p)
    {
        return (uint32_t)in->at((size_t)p) | ((uint32_t)in->at((size_t)p + 1) << 8) | ((uint32_t)in->at((size_t)p + 2) << 16)
               | ((uint32_t)in->at((size_t)p + 3) << 24);
    }
    void lit(uint32_t at, uint32_t v) { out->at(at) = (uint8_t)v; }
    void match(uint32_t at, uint32_t dist, uint32_t len)
    {
        for (uint32_t k = 0; k < len; k++) {
            out->at(at + k) = out->at(at + k - dist);
        }
    }
    void stored(uint32_t at, int64_t p, uint32_t len)
    {
        for (uint32_t k = 0; k < len; k++) {
            out->at(at + k) = in->at((size_t)p + k);
        }
    }
    int lane() { return 0; }
    int lanes() { return 1; }
    void sync() {}
};

static uint32_t sliced_crc(const std::vector<uint8_t> &d, uint32_t n)
{
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; i++) {
        tab[i] = lfq_crc_table_entry(i);
    }
    const uint32_t each = lfq_crc_slice_bytes(n);
    uint32_t total = 0;
    for (uint32_t s = 0; s < LFQ_CRC_SLICES; s++) {
        const uint32_t a = s * each < n ? s * each : n, b = a + each < n ? a + each : n;
        uint32_t c = 0xffffffffu;
        for (uint32_t i = a; i < b; i++) {
            c = tab[(c ^ d[i]) & 0xffu] ^ (c >> 8);
        }
        c = b > a ? ~c : 0u;
        total ^= lfq_crc_mul(lfq_crc_x8n(n - b), c);
    }
    return total;
}

int main(void)
{
    std::string line;
    static LfqInfTables T;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') {
            continue;
        }
        char *e;
        const unsigned long isize = strtoul(line.c_str(), &e, 10);
        if (isize > LFQ_INF_MAX_OUT) {
            return 2;
        }
        while (*e == ' ') {
            e++;
        }
        std::vector<uint8_t> in;
        if (*e != '-') {
            for (; e[0] && e[1]; e += 2) {
                const char b[3] = {e[0], e[1], 0};
                in.push_back((uint8_t)strtoul(b, nullptr, 16));
            }
        }
        std::vector<uint8_t> out(isize);
        HostIo io = {&in, &out};
        uint32_t n_out = 0;
        const int st = lfq_inflate(&T, 0, (int64_t)in.size(), (uint32_t)isize, &n_out, io);
        if (n_out > isize) {
            return 3;
        }
        std::string hex;
        static const char *dig = "0123456789abcdef";
        for (uint32_t i = 0; i < n_out; i++) {
            hex.push_back(dig[out[i] >> 4]);
            hex.push_back(dig[out[i] & 15]);
        }
        printf("%d %u %08x %s\n", st, n_out, sliced_crc(out, n_out), n_out ? hex.c_str() : "-");
    }
    return 0;
}
