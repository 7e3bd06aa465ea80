"""The topology of a device build (include/hpt.h, "device builds") restated in Python: integers throughout, float32 for the
cell of a centroid.  It is written another way round than the library -- bits interleaved one at a time, the radix tree cut
top-down by bisection instead of node by node -- and must give the child codes and the triangle ordinals of
hpt_bvh_device_build_host.  A plain module: no GPU, no tests."""
import bisect

import numpy as np

F32 = np.float32
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
MAX_LEAF_TRIS = 2
CELLS = 2097152
DEAD_KEY = (1 << 64) - 1


def dead(tr):
    with np.errstate(invalid="ignore", over="ignore"):
        e1 = tr["v1"].astype(F32) - tr["v0"].astype(F32)
        e2 = tr["v2"].astype(F32) - tr["v0"].astype(F32)
    return ~(np.isfinite(e1).all(axis=1) & np.isfinite(e2).all(axis=1))


def cells(tr):
    """[n, 3] cells of the live centroids (dead rows are zero) and the dead mask."""
    n = len(tr)
    is_dead = dead(tr)
    v = np.stack([tr["v0"], tr["v1"], tr["v2"]], axis=1).astype(F32)
    out = np.zeros((n, 3), np.int64)
    live = ~is_dead
    if not live.any():
        return out, is_dead
    mn, mx = v[live].min(axis=1), v[live].max(axis=1)              # a live triangle's coordinates are finite
    lo, hi = mn.min(axis=0), mx.max(axis=0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ext = (hi - lo).astype(F32)
        scale = np.where(ext > 0, F32(CELLS) / np.where(ext > 0, ext, F32(1)), F32(0)).astype(F32)
        c = (F32(0.5) * (mn + mx).astype(F32)).astype(F32)
        f = ((c - lo).astype(F32) * scale).astype(F32)
    inside = (f >= 1) & (f < CELLS)                                # a NaN fails both: cell 0
    cell = np.zeros(f.shape, np.int64)
    cell[inside] = f[inside].astype(np.int64)
    cell[(f >= 1) & ~(f < CELLS)] = CELLS - 1
    out[live] = cell
    return out, is_dead


def keys(tr):
    """The 64-bit key of every triangle as Python integers: bit k of x at 3k + 2, of y at 3k + 1, of z at 3k."""
    cell, is_dead = cells(tr)
    out = []
    for (x, y, z), d in zip(cell.tolist(), is_dead.tolist()):
        if d:
            out.append(DEAD_KEY)
            continue
        key = 0
        for k in range(21):
            key |= ((x >> k) & 1) << (3 * k + 2) | ((y >> k) & 1) << (3 * k + 1) | ((z >> k) & 1) << (3 * k)
        out.append(key)
    return out


def _leaf(first, count):
    return LEAF | first << 3 | (count - 1)


def build(tr, num_rounds):
    """dict(left, right: child codes per node, breadth-first; ordinals: per leaf slot; level_begin; depth)."""
    n = len(tr)
    key = keys(tr)
    order = sorted(range(n), key=lambda i: (key[i], i))
    ordinals = np.array([num_rounds + i for i in order], np.uint32).reshape(n)
    if n <= MAX_LEAF_TRIS:
        left = [_leaf(0, n) if n else EMPTY]
        return dict(left=np.array(left, np.uint32), right=np.array([EMPTY], np.uint32), ordinals=ordinals, level_begin=[0, 1], depth=1 if n else 0)
    # the sorted pairs as one integer each: the key above the 32-bit position; they ascend strictly
    aug = [key[i] << 32 | p for p, i in enumerate(order)]
    assert all(a < b for a, b in zip(aug, aug[1:]))

    def split(first, last):
        """The last position of the left half: the range is cut at the highest bit in which its ends differ."""
        bit = (aug[first] ^ aug[last]).bit_length() - 1
        return bisect.bisect_left(aug, aug[last] >> bit << bit, first, last + 1) - 1

    left, right, level_begin = [], [], []
    level = [(0, n - 1)]
    count = 1
    while level:
        level_begin.append(len(left))
        nxt = []
        for first, last in level:
            g = split(first, last)
            codes = []
            for a, b in ((first, g), (g + 1, last)):
                if b - a + 1 <= MAX_LEAF_TRIS:
                    codes.append(_leaf(a, b - a + 1))
                else:
                    codes.append(count)
                    count += 1
                    nxt.append((a, b))
            left.append(codes[0])
            right.append(codes[1])
        level = nxt
    level_begin.append(len(left))
    assert count == len(left)
    return dict(left=np.array(left, np.uint32), right=np.array(right, np.uint32), ordinals=ordinals, level_begin=level_begin, depth=len(level_begin) - 1)
