"""The targets of `lofreq call -l` (include/lofreq_amd.h: lfq_bed_*, lfq_set_bed): BED text parsed by the reference's rules, the
overlap predicate on the host, and the binding to a caller's context (SnvCaller.set_bed)."""
import ctypes as C

import numpy as np

from . import _lib


class BedError(ValueError):
    """lfq_bed_parse refused the text; .line is the 1-based line"""

    def __init__(self, line):
        ValueError.__init__(self, "BED text refused at line %d" % line)
        self.line = line


class Bed:
    """lfq_bed: the parsed targets.  Bed.parse(text) -> Bed; .names, .intervals(name), .overlap(name, beg, end)"""

    def __init__(self, h):
        self.h = h

    @staticmethod
    def parse(text):
        """text: bytes or str, already decompressed -> Bed; BedError where bed_read stops with a parse error"""
        if isinstance(text, str):
            text = text.encode("latin-1")
        L = _lib.load()
        h = C.c_void_p()
        bad = C.c_int64(0)
        rc = L.lfq_bed_parse(text, len(text), C.byref(h), C.byref(bad))
        if rc == -1 and bad.value > 0:      # LFQ_ERR_INVALID with a line: the text, not the call
            raise BedError(int(bad.value))
        _lib.check(rc, "lfq_bed_parse")
        return Bed(h)

    @property
    def names(self):
        L = _lib.load()
        return [L.lfq_bed_name(self.h, i).decode("latin-1") for i in range(L.lfq_bed_n_names(self.h))]

    def intervals(self, name):
        """-> (beg, end): int32 arrays in the table's order, sorted by (beg, end); empty for a name the BED does not hold"""
        beg, end, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int64(0)
        _lib.check(_lib.load().lfq_bed_intervals(self.h, name.encode("latin-1"), C.byref(beg), C.byref(end), C.byref(n)),
                   "lfq_bed_intervals")
        k = int(n.value)
        if k == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        return np.ctypeslib.as_array(beg, (k,)).copy(), np.ctypeslib.as_array(end, (k,)).copy()

    def overlap(self, name, beg, end):
        return bool(_lib.load().lfq_bed_overlap(self.h, name.encode("latin-1"), int(beg), int(end)))

    def close(self):
        if getattr(self, "h", None):
            _lib.load().lfq_bed_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_bed(caller, bed, name=None):
    """lfq_set_bed: the read sets this caller creates from now on take the table of `name` (bed=None: none again).  The context
    keeps its own copy, so `bed` may be closed afterwards."""
    L = _lib.load()
    if bed is None:
        _lib.check(L.lfq_set_bed(caller.h, None, None), "lfq_set_bed")
    else:
        _lib.check(L.lfq_set_bed(caller.h, bed.h, name.encode("latin-1") if name is not None else None), "lfq_set_bed")
