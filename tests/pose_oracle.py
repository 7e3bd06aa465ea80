"""The definition of a pose (include/hpt.h, "poses") restated in numpy float32, one operation at a time: a vertex
(x, y, z) of a triangle in part k, whose record has the rows r0, r1, r2 = (a, b, c, t), becomes

    X = ((r0.a * x + r0.b * y) + r0.c * z) + r0.t        and Y, Z likewise,

every product and every sum rounded to float32 on its own (numpy evaluates one ufunc at a time and fuses nothing).  Two
rules are tests on bits: a record whose 48 bytes are the identity's keeps the vertex's bits, and a vertex with a component
that is not finite becomes three words 0x7FC00000.  A plain module: no GPU, no library, no tests."""
import numpy as np

F32, U32 = np.float32, np.uint32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32).reshape(3, 4)
CANONICAL_NAN = 0x7FC00000


def _table(xforms):
    x = np.ascontiguousarray(xforms, F32)
    return x.reshape(-1, 3, 4)


def is_identity(xforms):
    """Per record: its 48 bytes are the identity's, +0 throughout."""
    x = _table(xforms)
    return (x.view(U32).reshape(len(x), 12) == IDENTITY.view(U32).reshape(12)).all(axis=1)


def raw(v, part, xforms):
    """The arithmetic alone, before the two rules: [n, 3, 3] float32."""
    v = np.ascontiguousarray(v, F32)
    r = _table(xforms)[np.asarray(part, np.int64)]                 # [n, 3, 4]
    x, y, z = v[..., 0], v[..., 1], v[..., 2]                      # [n, vertex]
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for a in range(3):
            ra = r[:, a, :]
            m0 = ra[:, 0, None] * x
            m1 = ra[:, 1, None] * y
            s = m0 + m1
            m2 = ra[:, 2, None] * z
            s = s + m2
            out[..., a] = s + ra[:, 3, None]
    assert out.dtype == F32
    return out


def pose_verts(v, part, xforms):
    """[n, 3, 3] float32 vertices (triangle, vertex, axis) posed by xforms[part[i]]."""
    v = np.ascontiguousarray(v, F32)
    part = np.asarray(part, np.int64)
    out = raw(v, part, xforms)
    bits = out.view(U32)
    bad = ((bits & 0x7F800000) == 0x7F800000).any(axis=-1)         # [n, vertex]
    bits[bad] = CANONICAL_NAN
    same = is_identity(xforms)[part]
    bits[same] = v.view(U32)[same]
    return out


def fused(v, part, xforms):
    """What a compiler that contracts multiply-add makes of the expression: a * x rounded, then two fused multiply-adds,
    then the sum with t.  A product of two float32 is exact in float64, so each fused step is one float64 sum rounded to
    float32.  No rules applied: compare with raw()."""
    v = np.ascontiguousarray(v, F32)
    r = _table(xforms)[np.asarray(part, np.int64)].astype(np.float64)
    x, y, z = (v[..., k].astype(np.float64) for k in range(3))
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for a in range(3):
            ra = r[:, a, :]
            s = (ra[:, 0, None] * x).astype(F32)
            s = (ra[:, 1, None] * y + s.astype(np.float64)).astype(F32)
            s = (ra[:, 2, None] * z + s.astype(np.float64)).astype(F32)
            out[..., a] = s + ra[:, 3, None].astype(F32)
    return out


def verts_of(tr):
    """The records' nine vertex floats as [n, 3, 3] float32, the same bits."""
    return np.ascontiguousarray(np.stack([tr["v0"], tr["v1"], tr["v2"]], axis=1), F32)


def with_verts(tr, v):
    """A copy of the records with the vertices v ([n, 3, 3] float32), bit for bit."""
    out = tr.copy()
    v = np.ascontiguousarray(v, F32)
    for k, name in enumerate(("v0", "v1", "v2")):
        out[name] = v[:, k]
    return out


def pose(tr, part, xforms):
    """The records after Scene.pose(xforms) on a scene whose rest pose is `tr`."""
    part = np.zeros(len(tr), np.int64) if part is None else part
    return with_verts(tr, pose_verts(verts_of(tr), part, xforms))
