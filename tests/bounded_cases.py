"""Case table of the bounded-build suites (include/hpt.h, "bounded device builds"): pairs of (records, max_depth).  The records
are device_build_cases' by import, and one more.  A plain module: no GPU, no tests.

  every SMALL case        at 0 (the limit, 30), need (forced from the root), need + 1 and (need + 30) // 2
  deep63                  at 0, 7 and 6 (need): its radix tree has 61 levels; at 0 the bounded tree has 30 at most and
                          does not fall back
  edge-2049               device_build_cases' _first(2049) at need: that mesh has 1872 triangles, so these are all of them
                          and need is 10; the forced levels grow to 468 nodes, across the 256-lane workgroup
  equal-64, tiny-0 .. 5   among the SMALL ones: equal keys at need; the one-node trees and the first inner children at 0
                          and 1 (tiny-5, which needs two levels, at 0 and 2)
  grid-stride             174 763 triangles at 0 and at need (17): the one big case
  REFUSED                 negative, 31, and need - 1
"""
import collections

import bounded_oracle as bo
import device_build_cases as dc

CASES = collections.OrderedDict(dc.CASES)
CASES["edge-2049"] = dc._bind(dc._first, 2049)

_RECORDS = {}
_TREES = {}


def records(name):
    """(L, sp, tr) of a case, once per process; callers must not write to them."""
    if name in dc.CASES:
        return dc.records(name)
    if name not in _RECORDS:
        L, sp, tr = CASES[name]()
        tr.setflags(write=False)
        _RECORDS[name] = (L, sp, tr)
    return _RECORDS[name]


def need_of(name):
    return bo.need(len(records(name)[2]))


def _depths(name):
    n = need_of(name)
    if name.startswith("tiny-"):
        return [0, 1] if n == 1 else [0, n]              # (five triangles need two levels: tiny-5 at 1 is among REFUSED)
    out = []
    for d in (0, n, n + 1, (n + 30) // 2):
        if d not in out and d <= 30:
            out.append(d)
    return out


PAIRS = [(name, d) for name in dc.SMALL if name != "deep63" for d in _depths(name)]
PAIRS += [("deep63", 0), ("deep63", 7), ("deep63", 6)]
PAIRS += [("edge-2049", need_of("edge-2049"))]
BIG_NEED = 17                                                       # need of 174 763 triangles (the suites assert it; not built at import)
BIG_PAIRS = [("grid-stride", 0), ("grid-stride", BIG_NEED)]
ALL_PAIRS = PAIRS + BIG_PAIRS
assert need_of("deep63") == 6 and need_of("edge-2049") == 10
assert ("equal-64", need_of("equal-64")) in PAIRS and ("tiny-0", 1) in PAIRS and ("tiny-5", 0) in PAIRS

# (case, max_depth) the call must refuse
REFUSED = [("edge-257", -1), ("edge-257", 31), ("edge-257", need_of("edge-257") - 1), ("deep63", 5), ("tiny-5", 1), ("tiny-3", -3)]


def pair_id(pair):
    return "%s@%d" % pair


def tree(hpt, name, max_depth):
    """The definition's tree of a pair (hpt_bvh_device_build_bounded_host: no device needed), once per process."""
    if (name, max_depth) not in _TREES:
        _TREES[(name, max_depth)] = hpt.device_build_bounded_bvh_host(*records(name), None, max_depth)
    return _TREES[(name, max_depth)]
