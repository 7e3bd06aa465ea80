"""The definition of a skin (include/hpt.h, "skinning") restated in numpy float32, one operation at a time, on top of
pose_oracle.raw: a corner with the rest vertex v and the influences (b_j, w_j), j = 0..3, of which those with non-zero
weight BITS are active, is

    keep    v's own bits, if every active influence's record has the identity's 48 bytes (or none is active);
    rigid   raw(v, record[b_j]), if exactly one influence is active and its weight has the bits of 1.0f;
    blend   acc = w_j * raw(v, record[b_j]) for the first active influence, acc = acc + w_j * raw(...) for each later
            one, in index order, every product and sum rounded to float32 on its own;

and after rigid and blend a vertex with a component that is not finite becomes three words 0x7FC00000.  The three cases
are masks on bits.  A plain module: no GPU, no library, no tests."""
import numpy as np

import pose_oracle as po

F32, U32 = np.float32, np.uint32
ONE = 0x3F800000
KEEP, RIGID, BLEND = 0, 1, 2


def _influences(v, bone, weight):
    v = np.ascontiguousarray(v, F32)
    n = len(v)
    return v, np.asarray(bone, np.int64).reshape(n, 3, 4), np.ascontiguousarray(weight, F32).reshape(n, 3, 4)


def _raw_corner(v, bone_j, xforms):
    """pose_oracle.raw with a record per CORNER: bone_j is [n, 3]."""
    n = len(v)
    return po.raw(v.reshape(n * 3, 1, 3), bone_j.reshape(n * 3), xforms).reshape(n, 3, 3)


def cases(bone, weight, xforms):
    """Per corner [n, 3]: KEEP, RIGID or BLEND, tested in that order."""
    bone = np.asarray(bone, np.int64)
    bone = bone.reshape(-1, 3, 4)
    wb = np.ascontiguousarray(weight, F32).reshape(-1, 3, 4).view(U32)
    active = wb != 0
    ident = po.is_identity(xforms)[bone]
    keep = (~active | ident).all(axis=-1)
    rigid = ~keep & (active.sum(axis=-1) == 1) & ((wb == ONE) & active).any(axis=-1)
    return np.where(keep, KEEP, np.where(rigid, RIGID, BLEND))


def _blend(v, bone, weight, xforms, row, fuse_sum):
    """acc over the active influences in index order; row(v, bone_j, xforms) gives p_j.  With fuse_sum every later step is
    one fused multiply-add: w_j * p_j exact in float64, added to acc, rounded once."""
    active = weight.view(U32) != 0
    acc = np.zeros_like(v)
    started = np.zeros(v.shape[:2], bool)
    with np.errstate(all="ignore"):
        for j in range(4):
            p = row(v, bone[..., j], xforms)
            w = weight[..., j, None]
            m = w * p
            if fuse_sum:
                s = (w.astype(np.float64) * p.astype(np.float64) + acc.astype(np.float64)).astype(F32)
            else:
                s = acc + m
            a = active[..., j]
            first, later = a & ~started, a & started
            acc[first] = m[first]
            acc[later] = s[later]
            started |= a
    assert acc.dtype == F32
    return acc


def raw(v, bone, weight, xforms):
    """The blend's arithmetic alone on every corner, before the cases and the non-finite rule: [n, 3, 3] float32."""
    v, bone, weight = _influences(v, bone, weight)
    return _blend(v, bone, weight, xforms, _raw_corner, False)


def skin_verts(v, bone, weight, xforms):
    """[n, 3, 3] float32 vertices (triangle, corner, axis) skinned by their influences over xforms."""
    v, bone, weight = _influences(v, bone, weight)
    kind = cases(bone, weight, xforms)
    out = _blend(v, bone, weight, xforms, _raw_corner, False)
    # rigid: the rows of the one active bone, no product with the weight
    active = weight.view(U32) != 0
    only = np.argmax(active, axis=-1)                                      # [n, 3]
    rigid = _raw_corner(v, np.take_along_axis(bone, only[..., None], axis=-1)[..., 0], xforms)
    out[kind == RIGID] = rigid[kind == RIGID]
    bits = out.view(U32)
    bad = ((bits & 0x7F800000) == 0x7F800000).any(axis=-1)
    bits[bad] = po.CANONICAL_NAN
    bits[kind == KEEP] = v.view(U32)[kind == KEEP]
    return out


def _fused_corner(v, bone_j, xforms):
    n = len(v)
    return po.fused(v.reshape(n * 3, 1, 3), bone_j.reshape(n * 3), xforms).reshape(n, 3, 3)


def fused(v, bone, weight, xforms, rows=True, blend=True):
    """What a compiler that contracts multiply-add makes of the blend: in the rows (pose_oracle.fused), in the sum
    acc + w_j * p_j, or both.  No cases, no rules applied: compare with raw()."""
    v, bone, weight = _influences(v, bone, weight)
    return _blend(v, bone, weight, xforms, _fused_corner if rows else _raw_corner, blend)


def skin(tr, bone, weight, xforms):
    """The records after Scene.skin(xforms) on a scene whose rest pose is `tr`."""
    return po.with_verts(tr, skin_verts(po.verts_of(tr), bone, weight, xforms))
