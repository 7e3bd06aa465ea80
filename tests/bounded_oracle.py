"""The topology of a bounded device build (include/hpt.h, "bounded device builds") restated in Python, another way round than
the library: the tree is built by recursion, depth first, from the keys of lbvh_oracle.py; a radix split is found by a
linear scan for the first position whose (key, position) pair has the top differing bit of the range's ends set; the
breadth-first numbers are given afterwards, by a walk over the finished tree.  It must give the child codes, the ordinals
and the counts of hpt_bvh_device_build_bounded_host.  A plain module: no GPU, no tests."""
import numpy as np

import lbvh_oracle as lo

MAX_BVH_DEPTH = 30
NONE_FORCED = 0xFFFFFFFF


def need(count):
    """The levels a range of `count` triangles takes at least: the smallest k >= 1 with 2^k >= (count + 1) // 2."""
    leaves = (count + 1) // 2
    k = 1
    while (1 << k) < leaves:
        k += 1
    return k


def effective_depth(nt, max_depth):
    """D, or None where the call is refused."""
    if max_depth == 0:
        return MAX_BVH_DEPTH
    if max_depth < 0 or max_depth > MAX_BVH_DEPTH or max_depth < need(nt):
        return None
    return max_depth


def build(tr, num_rounds, max_depth):
    """dict(left, right: child codes per node, breadth-first; ordinals: per leaf slot; level_begin; depth; max_depth;
    forced_nodes; first_forced_level)."""
    n = len(tr)
    D = effective_depth(n, max_depth)
    assert D is not None
    key = lo.keys(tr)
    order = sorted(range(n), key=lambda i: (key[i], i))
    ordinals = np.array([num_rounds + i for i in order], np.uint32).reshape(n)
    if n <= lo.MAX_LEAF_TRIS:
        left = [lo._leaf(0, n) if n else lo.EMPTY]
        return dict(left=np.array(left, np.uint32), right=np.array([lo.EMPTY], np.uint32), ordinals=ordinals, level_begin=[0, 1],
                    depth=1 if n else 0, max_depth=D, forced_nodes=0, first_forced_level=NONE_FORCED)
    aug = [key[i] << 32 | p for p, i in enumerate(order)]          # the key above the 32-bit position: strictly ascending
    forced_levels = []

    def node(first, count, d):
        """A subtree as a nested tuple (left, right); a leaf is its code."""
        if count <= lo.MAX_LEAF_TRIS:
            return lo._leaf(first, count)
        assert need(count) <= D - d
        if need(count) == D - d:
            forced_levels.append(d)
            leaves = (count + 1) // 2
            lc = 2 * ((leaves + 1) // 2)
        else:
            last = first + count - 1
            bit = (aug[first] ^ aug[last]).bit_length() - 1       # set in the last pair, clear in the first
            p = first
            while not (aug[p] >> bit) & 1:
                p += 1
            lc = p - first
        return (node(first, lc, d + 1), node(first + lc, count - lc, d + 1))

    root = node(0, n, 0)
    # breadth-first numbers: level by level, the inner children in order, left before right
    left, right, level_begin = [], [], []
    level, count = [root], 1
    while level:
        level_begin.append(len(left))
        nxt = []
        for nd in level:
            codes = []
            for ch in nd:
                if isinstance(ch, tuple):
                    codes.append(count)
                    count += 1
                    nxt.append(ch)
                else:
                    codes.append(ch)
            left.append(codes[0])
            right.append(codes[1])
        level = nxt
    level_begin.append(len(left))
    return dict(left=np.array(left, np.uint32), right=np.array(right, np.uint32), ordinals=ordinals, level_begin=level_begin,
                depth=len(level_begin) - 1, max_depth=D, forced_nodes=len(forced_levels),
                first_forced_level=min(forced_levels) if forced_levels else NONE_FORCED)
