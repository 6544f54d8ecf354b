/*
 * lfq_seg_items.h -- the work items of the row-segment kernels (lfq_dp_seg_kernel<0> and <1>), stated once for the
 * kernels that make them, the kernels that run them and the host check (lfq_seg_items_check.cpp).
 *
 * An item is one NEW row segment of one row-split column: segment r of record `slot` of class `cls`, phase1 <= r < n_seg
 * (segment 0 of a phase-1 record is the state the mid kernel had reached and is not run again).  Records of one class list
 * differ in n_seg - phase1 (lfq_split_plan answers 2..seg_max, a phase-1 record starts at r = 1), so no stride per record
 * enumerates them without holes.  Instead the items of a mode are LISTED: whoever appends a record to a class list also claims
 * n_seg - phase1 consecutive entries of the mode's item table (one atomic add on the mode's item counter) and writes the
 * packed (cls, slot, r) there.  Item i of a mode is entry i of its table, for 0 <= i < the counter: every existing pair once,
 * none that does not exist, no holes -- wavefront i runs item i, so the live wavefronts are a prefix of the launch whatever
 * the mix of n_seg and phase1.  A record that does not get its slot (the class list is full: slot >= per_class) is never
 * listed, claims nothing and runs unsplit.
 *
 * Modes as in the kernels: 0 = classes 0..1 (1 and 4 cells per lane), 1 = classes 2..4 (8, 16, 32).  The table has
 * LFQ_SEG_CLASSES * per_class * LFQ_SEG_MAX entries and lives behind the records (lfq_seg_items_of); mode 1's part starts where
 * mode 0's largest possible list ends.
 */
#ifndef LFQ_SEG_ITEMS_H
#define LFQ_SEG_ITEMS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define LFQ_SEG_HD __host__ __device__
#else
#define LFQ_SEG_HD
#endif

#ifndef LFQ_SEG_MAX
#define LFQ_SEG_MAX 8
#endif
#define LFQ_SEG_MODE0_CLASSES 2     /* classes 0..1 belong to mode 0, the rest to mode 1 */

LFQ_SEG_HD static inline int lfq_seg_mode_of(int cls)
{
    return cls >= LFQ_SEG_MODE0_CLASSES ? 1 : 0;
}

/* first entry of the mode's part of the item table */
LFQ_SEG_HD static inline int lfq_seg_items_base(int mode, int per_class)
{
    return mode ? LFQ_SEG_MODE0_CLASSES * per_class * LFQ_SEG_MAX : 0;
}

LFQ_SEG_HD static inline int32_t lfq_seg_item_pack(int cls, int slot, int r, int per_class)
{
    return (int32_t)((cls * per_class + slot) * LFQ_SEG_MAX + r);
}

/* item -> (class, record of the class list, segment); *rec = the record's index in LfqWork::longs */
LFQ_SEG_HD static inline void lfq_seg_item_unpack(int32_t item, int per_class, int *cls, int *slot, int *r, int *rec)
{
    *r = item % LFQ_SEG_MAX;
    *rec = item / LFQ_SEG_MAX;
    *cls = *rec / per_class;
    *slot = *rec % per_class;
}

/* The producer's half: record (cls, slot) with new segments phase1 .. n_seg - 1 got entries item0 .. of its mode's list.
 * Callers share the loop: `first` of `step` (one thread: 0 of 1; a wavefront: lane of 64). */
LFQ_SEG_HD static inline void lfq_seg_items_put(int32_t *table, int per_class, int item0, int cls, int slot, int phase1,
                                                int n_seg, int first, int step)
{
    int32_t *list = table + lfq_seg_items_base(lfq_seg_mode_of(cls), per_class);
    for (int j = first; j < n_seg - phase1; j += step) {
        list[item0 + j] = lfq_seg_item_pack(cls, slot, phase1 + j, per_class);
    }
}

#endif
