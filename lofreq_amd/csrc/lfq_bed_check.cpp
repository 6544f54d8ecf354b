/*
 * lfq_bed_check.cpp -- lfq_bed.h on the host, as a stand-alone program (tests/test_bed_edges.py compiles it with the host compiler,
 * plainly and sanitized; not part of the library).  One row per line of standard input, one answer per line of standard output:
 *
 *   <hex of the BED text, or -> <name> <beg:end,beg:end,... or ->
 *       ->   {"names":[[name,[[beg,end],...]],...],"overlap":[0|1,...]}   the tables in sorted order, the queries against <name>
 *       ->   {"error":<line>}                                               the text is refused at that line (1-based)
 *
 * The text lives in a vector of exactly its length, so a read beside it is the sanitizer's to find.
 */
#include <stdio.h>
#include <stdlib.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lfq_bed.h"

static int hexval(char ch)
{
    return ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
}

int main()
{
    std::string row;
    while (std::getline(std::cin, row)) {
        std::stringstream ss(row);
        std::string hex, name, queries;
        if (!(ss >> hex >> name >> queries)) {
            fprintf(stderr, "bad row\n");
            return 2;
        }
        std::vector<char> text;
        for (size_t i = 0; hex != "-" && i + 1 < hex.size(); i += 2) {
            const int hi = hexval(hex[i]), lo = hexval(hex[i + 1]);
            if (hi < 0 || lo < 0) {
                fprintf(stderr, "bad hex\n");
                return 2;
            }
            text.push_back((char)(hi * 16 + lo));
        }
        lfq_bed bed;
        int64_t bad = 0;
        if (!lfq_bed_parse_text(text.data(), (int64_t)text.size(), &bed, &bad)) {
            printf("{\"error\":%lld}\n", (long long)bad);
            continue;
        }
        printf("{\"names\":[");
        for (size_t t = 0; t < bed.names.size(); t++) {
            const LfqBedName &T = bed.names[t];
            printf("%s[\"%s\",[", t ? "," : "", T.name.c_str());
            for (size_t i = 0; i < T.beg.size(); i++) {
                printf("%s[%d,%d]", i ? "," : "", T.beg[i], T.end[i]);
            }
            printf("]]");
        }
        printf("],\"overlap\":[");
        const LfqBedName *T = bed.find(name.c_str());
        std::stringstream qs(queries == "-" ? "" : queries);
        std::string item;
        bool first = true;
        while (std::getline(qs, item, ',')) {
            const size_t colon = item.find(':');
            if (colon == std::string::npos) {
                fprintf(stderr, "bad query\n");
                return 2;
            }
            const int64_t beg = strtoll(item.c_str(), nullptr, 10), end = strtoll(item.c_str() + colon + 1, nullptr, 10);
            printf("%s%d", first ? "" : ",", T ? lfq_bed_tab_overlap(T->tab(), beg, end) : 0);
            first = false;
        }
        printf("]}\n");
    }
    return 0;
}
