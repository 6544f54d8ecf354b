/*
 * lfq_seg_items_check.cpp -- lfq_seg_items.h on the host, as a stand-alone program (tests/test_seg_items.py compiles it with the
 * host compiler; not part of the library).  It plays both halves of the rule the way the kernels do: records arrive in the
 * order given, each takes the next slot of its class list (a slot >= per_class is refused, as in lfq_long_reserve), claims its
 * entries of its mode's item list and writes them -- one thread for a record without a phase-1 stretch (the big prep kernel),
 * 64 lanes sharing the loop for one with it (the mid kernel); then every item of both modes is read back as
 * lfq_dp_seg_kernel reads it.
 *
 * Input, any number of scenarios:      S <per_class> <n>   followed by n lines   <cls> <n_seg> <phase1>
 * Output per scenario:                 M <mode> <items> <entries written outside [0, items)>      for mode 0 and 1
 *                                      I <mode> <item> <cls> <slot> <segment> <record index>      for every item, in order
 *                                      E
 */
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lfq_seg_items.h"

#define N_CLASSES 5         /* LFQ_SEG_CLASSES */

int main(void)
{
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        if (line[0] == '\n' || line[0] == '#') {
            continue;
        }
        long per_class = 0, n = 0;
        if (sscanf(line, "S %ld %ld", &per_class, &n) != 2 || per_class < 1 || per_class > 4096 || n < 0) {
            return 2;
        }
        std::vector<int32_t> table((size_t)N_CLASSES * (size_t)per_class * LFQ_SEG_MAX, -1);
        int n_cls[N_CLASSES] = {0, 0, 0, 0, 0}, n_items[2] = {0, 0};
        for (long i = 0; i < n; i++) {
            int cls = 0, n_seg = 0, phase1 = 0;
            if (!fgets(line, sizeof(line), stdin) || sscanf(line, "%d %d %d", &cls, &n_seg, &phase1) != 3 || cls < 0
                || cls >= N_CLASSES || phase1 < 0 || phase1 > 1 || n_seg - phase1 < 1 || n_seg > LFQ_SEG_MAX) {
                return 2;
            }
            const int slot = n_cls[cls]++;              /* the counter runs on past per_class, as on the device */
            if (slot >= per_class) {
                continue;                               /* no slot: the column runs unsplit and lists nothing */
            }
            const int mode = lfq_seg_mode_of(cls);
            const int item0 = n_items[mode];
            n_items[mode] += n_seg - phase1;
            if (phase1) {
                for (int lane = 0; lane < 64; lane++) {
                    lfq_seg_items_put(table.data(), (int)per_class, item0, cls, slot, phase1, n_seg, lane, 64);
                }
            } else {
                lfq_seg_items_put(table.data(), (int)per_class, item0, cls, slot, phase1, n_seg, 0, 1);
            }
        }
        for (int mode = 0; mode < 2; mode++) {
            const int base = lfq_seg_items_base(mode, (int)per_class);
            const int end = mode ? (int)table.size() : lfq_seg_items_base(1, (int)per_class);
            int stray = 0;
            for (int i = base + n_items[mode]; i < end; i++) {
                stray += table[(size_t)i] != -1;
            }
            printf("M %d %d %d\n", mode, n_items[mode], stray);
            for (int i = 0; i < n_items[mode]; i++) {
                int cls, slot, r, rec;
                lfq_seg_item_unpack(table[(size_t)(base + i)], (int)per_class, &cls, &slot, &r, &rec);
                printf("I %d %d %d %d %d %d\n", mode, i, cls, slot, r, rec);
            }
        }
        printf("E\n");
    }
    return 0;
}
