"""Rate of plp_summary's quality lines on a resident read set -> profiles/plp_quals_rate.json

  shape     the chain's region shape, the reads of profiles/readset_uniq_rate.py: 2 000 000 position-sorted reads of 150 bases
            over 1 Mb (300x), all-M, no BI / BD, no BAQ (the baq track is there and holds 255), no source quality
  roads     (a) lfq_plp_quals_from_tracks over all columns of the resident byte-nt tracks: lfq_plp_group_kernel + the copy of the
                grouped bytes into pinned memory, with the kernel's device time (lfq_last_plp_quals_times) and the bytes it reads
                and writes per second against the 6.29 TB/s copy ceiling the project uses.  Bytes, from the code: nt is read twice
                except for a column's first 64 observations (counted as twice: an upper bound of the traffic, a lower bound of
                nothing), bq / baq / mq once, three bytes written per observation, 8 + 40 bytes of offsets per column.
            (b) lfq_readset_pileup_snv + a synchronise, the call that makes those tracks, for scale
            (c) lfq_readset_pileup_indels with the all-columns switch off -- the default road, whose code is the parent's -- and
            (d) with the switch on
  timing    wall time of the calls from the host (C functions through ctypes, results on the host on return), after a warm-up:
            min and median of 7 per road.
  parent    `--indels-only OUT --tree DIR` measures road (c) alone with the package found under DIR (a build of the parent
            commit, run on the same box in the same job); `--parent-json OUT` folds those numbers into the result:
            c_within_parent_spread = |median(c) - median(parent)| <= the parent's own median - min.

    python profiles/plp_quals_rate.py [--parent-json FILE] [out.json]
    python profiles/plp_quals_rate.py --indels-only OUT.json [--tree DIR]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from readset_uniq_rate import GLEN, N_READS, REPS, RL, make_reads, stats, timed      # noqa: E402

COPY_CEILING_TBS = 6.29


def opt(args, name):
    return args[args.index(name) + 1] if name in args else None


def main():
    args = sys.argv[1:]
    indels_only, tree, parent_json = opt(args, "--indels-only"), opt(args, "--tree"), opt(args, "--parent-json")
    valued = {i + 1 for i, a in enumerate(args) if a in ("--indels-only", "--tree", "--parent-json")}
    rest = [a for i, a in enumerate(args) if not a.startswith("--") and i not in valued]
    sys.path.insert(0, os.path.abspath(tree) if tree else ROOT)
    import lofreq_amd as la
    from lofreq_amd import _lib
    L = _lib.load()
    cl = la.SnvCaller(0)
    rs = la.ReadSet.from_arrays(cl, make_reads())
    cols_p = C.POINTER(_lib.IndelColumnsC)()
    cp = np.zeros(GLEN, np.int64)

    def indels():
        _lib.check(L.lfq_readset_pileup_indels(cl.h, rs.h, 0, GLEN, 0, C.byref(cols_p), cp.ctypes.data), "lfq_readset_pileup_indels")

    if indels_only:
        res = {"tree": os.path.dirname(os.path.abspath(la.__file__)), "c_pileup_indels": stats(timed(indels))}
        print("c", res, flush=True)
        rs.close()
        cl.close()
        json.dump(res, open(indels_only, "w"), indent=1)
        return
    tr = _lib.Tracks()
    q_p = C.POINTER(_lib.PlpQualsC)()

    def snv():
        _lib.check(L.lfq_readset_pileup_snv(cl.h, rs.h, 0, GLEN, 3, C.byref(tr), cp.ctypes.data), "lfq_readset_pileup_snv")
        _lib.check(L.lfq_synchronize(cl.h), "lfq_synchronize")

    def quals():
        _lib.check(L.lfq_plp_quals_from_tracks(cl.h, C.byref(tr), 1, 0, tr.ncols, C.byref(q_p)), "lfq_plp_quals_from_tracks")

    res = {"shape": {"reads": N_READS, "read_len": RL, "span": GLEN, "depth": N_READS * RL // GLEN}, "reps": REPS}
    res["c_pileup_indels_switch_off"] = stats(timed(indels))
    print("c", res["c_pileup_indels_switch_off"], flush=True)
    cl.set_pileup_nt_packed(False)
    res["b_pileup_snv"] = stats(timed(snv))
    print("b", res["b_pileup_snv"], flush=True)
    t = timed(quals)
    st = la.last_plp_quals_times(cl)
    n_obs, n_cols = int(st.n_obs), int(st.n_cols)
    has_sq = bool(q_p.contents.sq)
    tracks_n = 3 + (1 if has_sq else 0)                      # bq, baq, mq (+ sq)
    read_b = n_obs * (2 + tracks_n) + n_cols * 8
    write_b = n_obs * tracks_n + n_cols * 40
    tbs = (read_b + write_b) / (st.kernel_ms * 1e-3) / 1e12
    res["a_plp_quals"] = dict(stats(t), kernel_ms=st.kernel_ms, n_cols=n_cols, n_obs=n_obs, n_launches=int(st.n_launches),
                              bytes_read=read_b, bytes_written=write_b, kernel_tb_per_s=tbs,
                              fraction_of_copy_ceiling=tbs / COPY_CEILING_TBS, copy_ceiling_tb_per_s=COPY_CEILING_TBS,
                              bytes_source="counted from the code, not from a counter run")
    print("a", res["a_plp_quals"], flush=True)
    res["a_over_b"] = res["a_plp_quals"]["median_ms"] / res["b_pileup_snv"]["median_ms"]
    cl.set_pileup_nt_packed(True)
    cl.set_indel_arrays_all_columns(True)
    res["d_pileup_indels_switch_on"] = stats(timed(indels))
    print("d", res["d_pileup_indels_switch_on"], flush=True)
    cl.set_indel_arrays_all_columns(False)
    res["d_over_c"] = res["d_pileup_indels_switch_on"]["median_ms"] / res["c_pileup_indels_switch_off"]["median_ms"]
    res["parent"] = None
    if parent_json:
        p = json.load(open(parent_json))["c_pileup_indels"]
        c = res["c_pileup_indels_switch_off"]
        spread = p["median_ms"] - p["min_ms"]
        res["parent"] = {"c_pileup_indels": p, "spread_ms": spread, "median_difference_ms": c["median_ms"] - p["median_ms"],
                         "c_within_parent_spread": abs(c["median_ms"] - p["median_ms"]) <= spread,
                         "source": "the parent commit's library, built apart, same box, same job"}
    rs.close()
    cl.close()
    out = rest[0] if rest else os.path.join(ROOT, "profiles", "plp_quals_rate.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("a_over_b", "d_over_c", "parent")}))


if __name__ == "__main__":
    main()
