"""Rate of plp_summary's header line on a resident read set -> profiles/plp_summary_rate.json

  shape     the chain's region shape, the reads of profiles/readset_uniq_rate.py: 2 000 000 position-sorted reads of 150 bases
            over 1 Mb (300x), all-M, no BI / BD
  roads     (a) lfq_readset_plp_summary over the whole span: the indel pileup it runs + lfq_plp_summary_kernel + the host's
                assembly, with the kernel's device time, the columns and the columns that took the ordered path
                (lfq_last_summary_times)
            (b) what a caller ran before for the same region: lfq_readset_pileup_snv + lfq_readset_pileup_indels + a synchronise
            (c) lfq_readset_pileup_indels alone: the part of (a) that is not new
  timing    wall time of the calls from the host (C functions through ctypes, results on the host on return), after a warm-up:
            min and median of 7 per road; the kernel time of (a) comes from device events.
  kernels   with --kernel-stats FILE (the kernel statistics CSV of a `rocprofv3 --kernel-trace --stats` run of
            `plp_summary_rate.py --trace-only`, taken in a run of its own): the average device time of the SNV pileup's count pass
            (lfq_pileup_tiles_kernel<false, ...>, which resolves the same (read, position) pairs) and of lfq_plp_summary_kernel
            in that run, and their ratio.  Without the file those entries are null: not measured.

    python profiles/plp_summary_rate.py [--trace-only] [--kernel-stats FILE] [out.json]
"""
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from readset_uniq_rate import GLEN, N_READS, REPS, RL, make_reads, stats, timed      # noqa: E402


def kernel_stats(path):
    """{kernel name: average ns} from a rocprofv3 kernel statistics CSV"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("Kernel_Name") or row.get("KernelName")
            avg = row.get("AverageNs") or row.get("Average") or row.get("AvgNs")
            if name and avg:
                out[name] = float(avg)
    return out


def main():
    import lofreq_amd as la
    from lofreq_amd import _lib
    args = sys.argv[1:]
    trace_only = "--trace-only" in args
    stats_csv = args[args.index("--kernel-stats") + 1] if "--kernel-stats" in args else None
    rest = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--kernel-stats")]
    L = _lib.load()
    cl = la.SnvCaller(0)
    rs = la.ReadSet.from_arrays(cl, make_reads())
    out_p = C.POINTER(_lib.PlpSummaryC)()
    cols_p = C.POINTER(_lib.IndelColumnsC)()
    tr = _lib.Tracks()
    cp = np.zeros(GLEN, np.int64)

    def summary():
        _lib.check(L.lfq_readset_plp_summary(cl.h, rs.h, 0, GLEN, 3, 0, C.byref(out_p)), "lfq_readset_plp_summary")

    def indels():
        _lib.check(L.lfq_readset_pileup_indels(cl.h, rs.h, 0, GLEN, 0, C.byref(cols_p), cp.ctypes.data), "lfq_readset_pileup_indels")

    def before():
        _lib.check(L.lfq_readset_pileup_snv(cl.h, rs.h, 0, GLEN, 3, C.byref(tr), cp.ctypes.data), "lfq_readset_pileup_snv")
        indels()
        _lib.check(L.lfq_synchronize(cl.h), "lfq_synchronize")

    if trace_only:                                           # under the profiler: a warm-up and three calls of each road
        for _ in range(4):
            summary()
            before()
        rs.close()
        cl.close()
        return
    res = {"shape": {"reads": N_READS, "read_len": RL, "span": GLEN, "depth": N_READS * RL // GLEN}, "reps": REPS}
    t = timed(summary)
    st = rs.last_summary_times()
    res["a_summary"] = dict(stats(t), kernel_ms=st.kernel_ms, n_cols=int(st.n_cols), n_ordered=int(st.n_ordered),
                            ordered_fraction=st.n_ordered / max(int(st.n_cols), 1), n_launches=int(st.n_launches))
    print("a", res["a_summary"], flush=True)
    res["b_pileup_snv_plus_indels"] = stats(timed(before))
    print("b", res["b_pileup_snv_plus_indels"], flush=True)
    res["c_pileup_indels"] = stats(timed(indels))
    print("c", res["c_pileup_indels"], flush=True)
    res["a_over_b"] = res["a_summary"]["median_ms"] / res["b_pileup_snv_plus_indels"]["median_ms"]
    res["a_minus_c_ms"] = res["a_summary"]["median_ms"] - res["c_pileup_indels"]["median_ms"]
    res["kernels"] = {"snv_count_pass_avg_ms": None, "summary_kernel_avg_ms": None, "summary_over_count_pass": None,
                      "source": "not measured"}
    if stats_csv:
        ks = kernel_stats(stats_csv)
        cnt = [v for k, v in ks.items() if "lfq_pileup_tiles_kernel" in k and "256" in k]      # <false, 256>: the count pass
        smk = [v for k, v in ks.items() if "lfq_plp_summary_kernel" in k]
        if cnt and smk:
            res["kernels"] = {"snv_count_pass_avg_ms": cnt[0] / 1e6, "summary_kernel_avg_ms": smk[0] / 1e6,
                              "summary_over_count_pass": smk[0] / cnt[0],
                              "source": "rocprofv3 --kernel-trace --stats, a run of its own (--trace-only)"}
        res["kernels"]["names_seen"] = sorted(k for k in ks if "pileup" in k or "plp" in k)
    rs.close()
    cl.close()
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "plp_summary_rate.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("a_over_b", "a_minus_c_ms", "kernels")}))


if __name__ == "__main__":
    main()
