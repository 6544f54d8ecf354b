"""Plain restatement of `lofreq call -l` (bedidx.c's bed_read and bed_overlap, and where plp.c applies them), written from the
rules in include/lofreq_amd.h, not from the library's code.  Shared by tests/test_bed_model.py, tests/test_bed_edges.py,
tests/test_abi_bed.py and tests/test_gpu_bed.py.

  parse(text)        -> {name: [(beg, end), ...] sorted by (beg, end)}, names in order of first appearance; BedRefused(line)
  overlap(iv, b, e)  -> some interval has end_i > b and beg_i < e
  keep_reads / keep_columns / bed_then_cap: the read rule (plp.c:625-629), the column rule (plp.c:1412), and -d on the survivors
"""
import re

import numpy as np

import maxdepth_model as mm

INT32_MAX = (1 << 31) - 1
SPACE = " \t\n\v\f\r"
_U = re.compile(r"[ \t\n\v\f\r]*([+-]?)([0-9]+)")


class BedRefused(Exception):
    def __init__(self, line):
        Exception.__init__(self, "line %d" % line)
        self.line = line


def _scan_u(s, at):
    """sscanf's %u -> (the number as written, sign applied; where it ends), or None"""
    m = _U.match(s, at)
    if not m:
        return None
    v = int(m.group(2))
    return (-v if m.group(1) == "-" else v), m.end()


def parse(text):
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    out = {}
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()                                     # the text ends with its last newline
    for no, line in enumerate(lines, 1):
        if line == "":
            break                                       # an empty line ends the file, silently
        line = line.split("\0")[0]
        body = line.lstrip(SPACE)
        if body == "" or body[0] == "#":
            continue
        k = 0
        while k < len(body) and body[k] not in SPACE:
            k += 1
        name, nums = body[:k], []
        if k < len(body):
            a = _scan_u(body, k + 1)
            if a:
                nums.append(a[0])
                b = _scan_u(body, a[1])
                if b:
                    nums.append(b[0])
        bad = not nums
        if len(nums) == 1:
            beg, end = nums[0] - 1, nums[0]            # the 1-based position list
            bad = nums[0] <= 0                          # 0 wraps around in the reference: end < beg; a negative number is huge
        elif len(nums) == 2:
            beg, end = nums
            bad = beg < 0 or end < 0 or end < beg       # a negative number is a huge unsigned one: refused either way
        if not bad and (beg > INT32_MAX or end > INT32_MAX):
            bad = True                                  # the stated departure
        if bad:
            if name in ("browser", "track"):
                continue
            raise BedRefused(no)
        out.setdefault(name, []).append((beg, end))
    return {k: sorted(v) for k, v in out.items()}


def overlap(iv, beg, end):
    return any(e > beg and b < end for b, e in iv)


def endpos(pos0, cigar):
    """bam_endpos; cigar = [(op, len)]"""
    n = sum(l for op, l in cigar if op in "MDN=X")
    return pos0 + (n if n > 0 else 1)


def keep_reads(iv, pos, ends):
    return np.array([1 if overlap(iv, int(p), int(e)) else 0 for p, e in zip(pos, ends)], np.uint8)


def keep_columns(iv, col_pos):
    return np.array([overlap(iv, int(p), int(p) + 1) for p in col_pos], bool)


def bed_then_cap(iv, pos, ends, max_depth, cap_ends=None):
    """BED first; bam_plp_push's rule (tests/maxdepth_model.py) then sees the survivors in file order; None: no cap.  cap_ends:
    the ends that rule counts with (maxdepth_model.ref_end, which has no + 1 for a read without reference bases), else `ends`"""
    keep = keep_reads(iv, pos, ends)
    if max_depth is None:
        return keep
    idx = np.nonzero(keep)[0]
    ce = ends if cap_ends is None else cap_ends
    sub = mm.kept([pos[i] for i in idx], [ce[i] for i in idx], max_depth)
    out = np.zeros(len(pos), np.uint8)
    out[idx[sub.astype(bool)]] = 1
    return out
