"""What lfq_readset_baq_fill saves: one C4-shaped region -- 400 000 position-sorted reads of 150 bases at
500x that follow the contig with 1 % mismatches, every 25th with a one-base deletion, BI / BD in every record -- through

  all_stored   lfq_readset_create_from_bam_tags + lfq_readset_baq_fill, every read carries lb and the deletion reads ad: what the
               pipeline bwa -> viterbi -> alnqual -> indelqual hands to `call`
  none_stored  the same two calls on the records without lb / ai / ad
  recompute    lfq_readset_create_from_bam + lfq_readset_baq on the tagged records: the road without the tag reuse
  decode_plain lfq_readset_create_from_bam alone on the tagged records (the decode without the stored-tag pass)

each REPS times after a warm-up, alternating; per call the device's own clocks (lfq_last_bam_decode_times, lfq_last_baq_fill_stats,
lfq_last_baq_times) and the wall time from the first call until the context is idle.  Writes tag_reuse_rate.json into the directory
given (default: profiles/).

    python profiles/tag_reuse_rate.py [output directory]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, RL, DEPTH, REPS, L_QNAME = 400000, 150, 500, 5, 24


def make_records(tags, seed=812):
    rng = np.random.default_rng(seed)
    glen = N * RL // DEPTH + RL + 8
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), glen)
    pos = (np.arange(N, dtype=np.int64) * RL // DEPTH).astype(np.int32)
    dele = np.arange(N) % 25 == 0
    code = np.zeros(256, np.uint8)
    code[list(b"ACGT")] = (1, 2, 4, 8)
    sizes = np.zeros(N, np.int64)
    blocks = {}
    for cls in (False, True):
        idx = np.flatnonzero(dele == cls)
        m = len(idx)
        at = pos[idx][:, None] + np.arange(RL)[None, :] + (cls * (np.arange(RL) >= 75))[None, :]     # 75M1D75M skips one base
        letters = ref[at]
        mm = rng.random((m, RL)) < 0.01
        letters = np.where(mm, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (m, RL))], letters)
        nib = code[letters]
        cig = np.asarray([75 << 4, (1 << 4) | 2, 75 << 4] if cls else [RL << 4], "<u4").view(np.uint8)
        z = lambda tag, lo, hi: [np.tile(np.frombuffer(tag + b"Z", np.uint8), (m, 1)),
                                 (33 + rng.integers(lo, hi, (m, RL), dtype=np.uint8)).astype(np.uint8), np.zeros((m, 1), np.uint8)]
        name = np.zeros((m, L_QNAME), np.uint8)
        name[:, :4] = np.frombuffer(b"read", np.uint8)
        fields = [name, np.tile(cig, (m, 1)), (nib[:, 0::2] << 4 | nib[:, 1::2]).astype(np.uint8),
                  rng.integers(20, 42, (m, RL), dtype=np.uint8)] + z(b"BI", 30, 60) + z(b"BD", 30, 60)
        if tags:
            fields += z(b"lb", 20, 60) + (z(b"ad", 20, 60) if cls else [])
        blocks[cls] = (idx, np.ascontiguousarray(np.concatenate(fields, axis=1)))
        sizes[idx] = blocks[cls][1].shape[1]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    data = np.zeros(int(off[-1]), np.uint8)
    for idx, blk in blocks.values():
        data[(off[idx][:, None] + np.arange(blk.shape[1])[None, :]).reshape(-1)] = blk.reshape(-1)
    return {"data": data, "data_off": off, "pos": pos, "flag": ((np.arange(N) & 1) << 4).astype(np.uint16), "mapq": np.full(N, 60, np.uint8),
            "l_qname": np.full(N, L_QNAME, np.uint16), "n_cigar": np.where(dele, 3, 1).astype(np.uint32),
            "l_qseq": np.full(N, RL, np.int32), "ref": ref.tobytes()}


def one(la, cl, R, read_tags, fill, baq=True):
    cl.synchronize()
    t0 = time.perf_counter()
    rs = la.ReadSet.from_bam_records(cl, R["data"], R["data_off"], R["pos"], R["flag"], R["mapq"], R["l_qname"], R["n_cigar"],
                                     R["l_qseq"], R["ref"], read_tags=read_tags)
    t1 = time.perf_counter()
    if fill:
        rs.baq_fill(extended=True, idaq=True)
    elif baq:
        rs.baq(extended=True, idaq=True)
    cl.synchronize()
    t2 = time.perf_counter()
    d = la.last_bam_decode_times(cl)
    out = {"wall_ms": (t2 - t0) * 1e3, "create_wall_ms": (t1 - t0) * 1e3, "baq_wall_ms": (t2 - t1) * 1e3, "decode_upload_ms": d["upload_ms"],
           "decode_kernels_ms": d["kernels_ms"], "decode_download_ms": d["download_ms"], "decode_launches": d["n_launches"]}
    if fill:
        s = la.last_baq_fill_stats(cl)
        out.update(hmm_ms=s["ms_hmm"], merge_ms=s["ms_merge"], n_need_hmm=s["n_need_hmm"], n_hmm_launches=s["n_hmm_launches"])
    elif baq:
        b = cl.baq_times()
        out.update(hmm_ms=b["ms_kernels"], merge_ms=0.0, n_need_hmm=b["n_reads"], n_hmm_launches=b["n_launches"])
    rs.close()
    return out


def main():
    import lofreq_amd as la
    cl = la.SnvCaller(0)
    tagged, bare = make_records(True), make_records(False)
    roads = {"all_stored": (tagged, 3, True, True), "none_stored": (bare, 3, True, True), "recompute": (tagged, 0, False, True),
             "decode_plain": (tagged, 0, False, False)}
    runs = {k: [] for k in roads}
    for rep in range(REPS + 1):
        for k, (R, tags, fill, baq) in roads.items():
            r = one(la, cl, R, tags, fill, baq)
            if rep:                         # the first pass warms allocations and the code objects up
                runs[k].append(r)
    res = {"n_reads": N, "read_length": RL, "depth": DEPTH, "reps": REPS, "record_bytes": {"tagged": int(tagged["data_off"][-1]) // N,
                                                                                          "bare": int(bare["data_off"][-1]) // N}}
    for k, v in runs.items():
        res[k] = {f: {"median": float(np.median([x[f] for x in v])), "min": float(min(x[f] for x in v)), "max": float(max(x[f] for x in v))}
                  for f in v[0]}
    cl.close()
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    json.dump(res, open(os.path.join(out_dir, "tag_reuse_rate.json"), "w"), indent=1)
    for k in roads:
        print(k, {f: round(res[k][f]["median"], 3) for f in res[k]})


if __name__ == "__main__":
    main()
