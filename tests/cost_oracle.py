"""The tree cost of include/hpt.h ("tree cost"), restated in numpy over the arrays export_bvh_host, refit_bvh_host and
Scene.export_bvh return.  The sums are uint64 (every term is below 2^35 and a tree has fewer than 2^24 nodes, so nothing
wraps) and returned as Python integers; the doubles are Python floats -- IEEE double, one operation at a time, in the order
the header writes them, which is the order the library's one composing function evaluates them in, so they are compared bit
for bit.  A plain module: no GPU, no tests."""
import struct

import numpy as np

EMPTY, LEAF = 0xFFFFFFFF, 0x80000000
INT_KEYS = ("inner_children", "leaf_children", "empty_children", "leaf_slots", "inner_xy", "inner_yz", "inner_zx", "leaf_xy", "leaf_yz", "leaf_zx")
DOUBLE_KEYS = ("box_visits", "tri_tests", "sah")
KEYS = INT_KEYS + ("root_extent", "num_nodes") + DOUBLE_KEYS


def _planes(q, c):
    """lo[n, 3], hi[n, 3] of child c: word 2a holds the lower planes (left child in the low half), word 2a + 1 the upper."""
    w = q[:, :6].astype(np.uint64)
    half = (w >> np.uint64(16)) if c else (w & np.uint64(0xFFFF))
    return half[:, 0::2], half[:, 1::2]


def cost(bvh) -> dict:
    q = np.ascontiguousarray(bvh["qnodes"], np.uint32).reshape(-1, 8)
    n = len(q)
    out = dict.fromkeys(INT_KEYS, 0)
    root_lo, root_hi, root_any = [0xFFFF] * 3, [0] * 3, False
    for c in (0, 1):
        code = q[:, 6 + c]
        lo, hi = _planes(q, c)
        d = np.where(hi >= lo, hi - lo, np.uint64(0))
        empty = code == EMPTY
        leaf = ~empty & ((code & LEAF) != 0)
        inner = ~empty & ~leaf
        k = ((code & 7) + 1).astype(np.uint64)
        xy, yz, zx = d[:, 0] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 0]
        out["empty_children"] += int(empty.sum())
        out["leaf_children"] += int(leaf.sum())
        out["inner_children"] += int(inner.sum())
        out["leaf_slots"] += int(k[leaf].sum())
        for key, t in (("xy", xy), ("yz", yz), ("zx", zx)):
            out["leaf_" + key] += int((k[leaf] * t[leaf]).sum(dtype=np.uint64))
            out["inner_" + key] += int(t[inner].sum(dtype=np.uint64))
        if n and not empty[0]:
            root_any = True
            for a in range(3):
                root_lo[a] = min(root_lo[a], int(lo[0, a]))
                root_hi[a] = max(root_hi[a], int(hi[0, a]))
    assert all(v < 1 << 60 for v in out.values())
    out["root_extent"] = tuple(root_hi[a] - root_lo[a] if root_any and root_hi[a] >= root_lo[a] else 0 for a in range(3))
    out["num_nodes"] = n
    s = [float(np.float32(v)) for v in bvh["qscale"]]
    Axy, Ayz, Azx = s[0] * s[1], s[1] * s[2], s[2] * s[0]
    rx, ry, rz = (float(v) for v in out["root_extent"])
    root_area = rx * ry * Axy + ry * rz * Ayz + rz * rx * Azx
    if root_area > 0.0:
        out["box_visits"] = 1.0 + (float(out["inner_xy"]) * Axy + float(out["inner_yz"]) * Ayz + float(out["inner_zx"]) * Azx) / root_area
        out["tri_tests"] = (float(out["leaf_xy"]) * Axy + float(out["leaf_yz"]) * Ayz + float(out["leaf_zx"]) * Azx) / root_area
        out["sah"] = 2.0 * out["box_visits"] + out["tri_tests"]
    else:
        out["box_visits"] = out["tri_tests"] = out["sah"] = 0.0
    return out


def pack(c) -> bytes:
    """The 120 bytes of hpt_tree_cost holding these values."""
    return struct.pack("<10Q4I3d", *[c[k] for k in INT_KEYS], *c["root_extent"], c["num_nodes"], *[c[k] for k in DOUBLE_KEYS])


def same(what, got, want):
    """Every field equal -- the doubles bit for bit -- and, where `got` carries the struct's bytes, those too."""
    for k in KEYS:
        g, w = got[k], want[k]
        if k in DOUBLE_KEYS:
            g, w = struct.pack("<d", g), struct.pack("<d", w)
        assert g == w, "%s: %s is %r, expected %r" % (what, k, got[k], want[k])
    if "bytes" in got:
        assert got["bytes"] == (want["bytes"] if "bytes" in want else pack(want)), what + ": the struct's bytes"
