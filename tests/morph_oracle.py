"""The definition of a morph (include/hpt.h, "morph targets") restated in numpy float32, one operation at a time.  Target t
owns the entries target_begin[t] .. target_begin[t + 1] - 1; entry e moves corner entry_corner[e] by entry_delta[e].  A
target is ACTIVE if its weight is neither +0 nor -0, that is (bits << 1) != 0.  A corner with the rest vertex v is

    keep    v's own bits, if no active target has an entry for it;
    morph   acc = v, and for each active target that has an entry for it, in ascending target order, acc = acc + w_t * d,
            the product rounded to float32, then the sum;

and after morph a vertex with a component that is not finite becomes three words 0x7FC00000.  Active, keep and the
non-finite rule are masks on bits.  A plain module: no GPU, no library, no tests."""
import numpy as np

import pose_oracle as po

F32, U32 = np.float32, np.uint32


def arrays(target_begin, entry_corner, entry_delta):
    tb = np.asarray(target_begin, np.int64).reshape(-1)
    ec = np.asarray(entry_corner, np.int64).reshape(-1)
    ed = np.ascontiguousarray(entry_delta, F32).reshape(-1, 3)
    assert tb[0] == 0 and tb[-1] == len(ec) == len(ed) and (np.diff(tb) >= 0).all()
    return tb, ec, ed


def active(weights):
    """Per target: the weight is neither +0 nor -0."""
    bits = np.ascontiguousarray(weights, F32).reshape(-1).view(U32)
    return ((bits << U32(1)) & U32(0xFFFFFFFF)) != 0


def _sum(v, tb, ec, ed, w, fuse, descending):
    """(acc [n * 3, 3] float32, touched [n * 3] bool): the sum over the active targets, one target at a time.  With `fuse`
    every step is one fused multiply-add: w * d exact in float64, added to acc, rounded once.  With `descending` the targets
    are taken from the last to the first."""
    acc = np.ascontiguousarray(v, F32).reshape(-1, 3).copy()
    touched = np.zeros(len(acc), bool)
    on = active(w)
    order = range(len(tb) - 1)
    with np.errstate(all="ignore"):
        for t in (reversed(order) if descending else order):
            if not on[t]:
                continue                                           # never evaluated
            c, d = ec[tb[t]:tb[t + 1]], ed[tb[t]:tb[t + 1]]
            assert (np.diff(c) > 0).all()                          # strictly ascending: each corner once
            wt = F32(w[t])
            if fuse:
                acc[c] = (np.float64(wt) * d.astype(np.float64) + acc[c].astype(np.float64)).astype(F32)
            else:
                m = wt * d
                assert m.dtype == F32
                acc[c] = acc[c] + m
            touched[c] = True
    assert acc.dtype == F32
    return acc, touched


def raw(v, target_begin, entry_corner, entry_delta, weights, fuse=False, descending=False):
    """The sum alone on every corner, before keep and the non-finite rule: [n, 3, 3] float32.  fuse: what a compiler that
    contracts multiply-add makes of it; descending: what a walk in the wrong order makes of it."""
    tb, ec, ed = arrays(target_begin, entry_corner, entry_delta)
    w = np.ascontiguousarray(weights, F32).reshape(-1)
    assert len(w) == len(tb) - 1
    acc, _ = _sum(v, tb, ec, ed, w, fuse, descending)
    return acc.reshape(-1, 3, 3)


def morph_verts(v, target_begin, entry_corner, entry_delta, weights, fuse=False, descending=False):
    """[n, 3, 3] float32 vertices (triangle, corner, axis) morphed by the targets under `weights`."""
    v = np.ascontiguousarray(v, F32)
    tb, ec, ed = arrays(target_begin, entry_corner, entry_delta)
    w = np.ascontiguousarray(weights, F32).reshape(-1)
    assert len(w) == len(tb) - 1
    acc, touched = _sum(v, tb, ec, ed, w, fuse, descending)
    bits = acc.view(U32)
    bad = ((bits & 0x7F800000) == 0x7F800000).any(axis=-1)
    bits[bad] = po.CANONICAL_NAN
    keep = ~touched
    bits[keep] = v.reshape(-1, 3).view(U32)[keep]
    return acc.reshape(-1, 3, 3)


def morph(tr, target_begin, entry_corner, entry_delta, weights, **kw):
    """The records after Scene.morph(weights) on a scene without a deformer whose rest pose is `tr`."""
    return po.with_verts(tr, morph_verts(po.verts_of(tr), target_begin, entry_corner, entry_delta, weights, **kw))
