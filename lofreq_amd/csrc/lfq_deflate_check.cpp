/*
 * lfq_deflate_check.cpp -- lfq_deflate.h on the host, as a stand-alone program (tests/test_deflate_edges.py compiles it with the
 * host compiler; not part of the library).  One payload per line of standard input, one answer per line of standard output:
 *
 *   <hex of the payload>   ->   <block type> <hex of the stream> <crc32 of the payload, hex> <1 if lfq_inflate.h gives it back, else 0>
 *
 * The compressor runs with lanes() = 1, so every step of 64 positions is walked one position at a time.  The payload vector holds
 * exactly the payload and the stream vector exactly the dwords that hold 5 + n bytes, and every access goes through vector::at:
 * one beside them ends the program, sanitized or not.  The CRC is computed as the device computes it, in 64 slices.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "lfq_deflate.h"

struct DefIo {
    const std::vector<uint8_t> *in;
    std::vector<uint8_t> *out;
    int lane() { return 0; }
    int lanes() { return 1; }
    void sync() {}
    bool any(bool v) { return v; }
    uint32_t ld8(uint32_t p) { return in->at(p); }
    uint32_t ld32(uint32_t p)
    {
        return (uint32_t)in->at(p) | ((uint32_t)in->at(p + 1) << 8) | ((uint32_t)in->at(p + 2) << 16) | ((uint32_t)in->at(p + 3) << 24);
    }
    void out32(uint32_t w, uint32_t v)
    {
        for (uint32_t k = 0; k < 4; k++) {
            out->at(4 * (size_t)w + k) = (uint8_t)(v >> (8 * k));
        }
    }
    void add32(uint32_t *p, uint32_t v) { *p += v; }
    void or32(uint32_t *p, uint32_t v) { *p |= v; }
};

struct InfIo {
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
    static LfqDefState S;
    static LfqInfTables T;
    static const char *dig = "0123456789abcdef";
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') {
            continue;
        }
        std::vector<uint8_t> in;
        for (const char *e = line.c_str(); e[0] && e[1]; e += 2) {
            const char b[3] = {e[0], e[1], 0};
            in.push_back((uint8_t)strtoul(b, nullptr, 16));
        }
        if (in.empty() || in.size() > LFQ_DEF_MAX_IN) {
            return 2;
        }
        const uint32_t n = (uint32_t)in.size();
        std::vector<uint8_t> stream(((size_t)5 + n + 3) / 4 * 4);
        memset(&S, 0xa5, sizeof(S));            /* nothing of the state may be taken for granted */
        DefIo io = {&in, &stream};
        const LfqDefResult R = lfq_deflate(&S, n, io);
        if (R.n_bytes > 5 + n) {
            return 3;
        }
        stream.resize(R.n_bytes);
        std::vector<uint8_t> back(n);
        InfIo inf = {&stream, &back};
        uint32_t n_back = 0;
        const int st = lfq_inflate(&T, 0, (int64_t)stream.size(), n, &n_back, inf);
        const int same = st == LFQ_INF_OK && n_back == n && memcmp(back.data(), in.data(), n) == 0;
        std::string hex;
        for (uint8_t v : stream) {
            hex.push_back(dig[v >> 4]);
            hex.push_back(dig[v & 15]);
        }
        printf("%u %s %08x %d\n", R.btype, hex.c_str(), sliced_crc(in, n), same);
    }
    return 0;
}
