"""Case table of the pose suite (include/hpt.h, "poses"): a base scene and a sequence of steps on ONE live handle.  It
builds on refit_cases' helpers and renders as it does: 48 x 48, depth 4, 4 spp, seed 31, the Cornell camera.  A plain
module: no GPU, no tests.

A step is one of
    ("parts", tri_part, num_parts)     Scene.set_parts: a part per triangle, and the rest pose is what the scene holds now
    ("pose", xforms)                   Scene.pose: [num_parts, 3, 4] float32, absolute, applied to the rest pose
    ("tris", records)                  Scene.update_triangles: the rest pose becomes these records' vertices
    ("dverts", records)                Scene.update_vertices_device with these records' 36 vertex bytes; the same rule
and expected(name)[i] are the records the handle holds after step i, by pose_oracle.  The base is
banded(cornell_with_sphere(2000)) -- 12 wall triangles, part 0, and the 1860-triangle sphere, part 1 -- unless said
otherwise:

  identity        every part at identity: the tree stays the builder's bytes and read_triangles gives the input's bytes.
                  One wall vertex coordinate of the base is -0.0, which the arithmetic would turn into +0.0
  turn            part 1 turned 30, 60 and 90 degrees about the sphere's centre (the tilted axis of refit_cases' turn), as
                  absolute poses
  out             part 1 scaled sixfold and moved three scene extents out of the old grid (refit_cases' out, its camera)
  shrink          both parts scaled by 0.25 about the look-at point
  shear-mirror    part 1 sheared, then reflected (determinant -1): the frames must follow
  die-and-return  a NaN entry in part 1's record; back to a finite pose; an infinity in part 0's record; part 1 scaled by
                  1e38 and pushed by 3.3e38 along z, so that every Z overflows to infinity and the vertex reaches the
                  canonical NaN by arithmetic; every part dead; all back at identity
  per-triangle    cornell_random_triangles(3000) with scramble's enlargement, 3001 parts: the walls are part 0, every
                  random triangle has a part and a seeded rigid transform of its own (the last two share one), and the
                  last part owns no triangle.  More parts than the kernel stages in LDS: the table is read from memory
  tiny-1, -2, -3  scenes of 1, 2 and 3 triangles, a part per triangle, posed twice
  edges-85, edges-171, edges-256
                  the first 85, 171 and 256 triangles of the base.  k_pose_verts runs one lane per VERTEX in workgroups
                  of 256: 85 triangles are 255 lanes (the last workgroup one lane short), 171 are 513 (one lane over two
                  full workgroups) and 256 are 768 (the last workgroup exactly full; no multiple of three is 256)
  interleave      pose, update_triangles, pose, update_vertices_device, pose, set_parts with another map, pose: the
                  rest-pose rule at every joint
  dv-turn, dv-die-and-return, dv-tiny-1, -2, -3
                  the steps of refit_cases' cases of those names fed through update_vertices_device: the trees must be
                  update_triangles' (refit_cases.tree)"""
import collections

import numpy as np

import pose_oracle as po
import refit_cases as rc
from path_tracing_amd import scene_io as sio

F32 = np.float32
W, H, DEPTH, SPP, SEED = rc.W, rc.H, rc.DEPTH, rc.SPP, rc.SEED
NWALL = rc.NWALL
Case = collections.namedtuple("Case", "name make")
Data = collections.namedtuple("Data", "L sp tr steps order eye look", defaults=(sio.CORNELL_EYE, sio.CORNELL_LOOK))
NAN, INF = float("nan"), float("inf")


# ---- 3 x 4 records, built in double and rounded once -------------------------------------------------------------------

def identity(n=1):
    return np.tile(po.IDENTITY, (n, 1, 1)).astype(F32)


def affine(M, centre=(0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0)):
    """x -> M (x - centre) + centre + shift as a record."""
    M, c = np.asarray(M, np.float64), np.asarray(centre, np.float64)
    r = np.zeros((3, 4))
    r[:, :3] = M
    r[:, 3] = c - M @ c + np.asarray(shift, np.float64)
    return r.astype(F32)


def rot_y(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def rot_z(deg):
    a = np.radians(deg)
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def tilted(deg):
    return rot_z(deg) @ rot_y(deg)


def table(*records):
    return np.stack([np.asarray(r, F32) for r in records]).astype(F32)


def two_parts(n, nwall=NWALL):
    p = np.ones(n, np.int32)
    p[:nwall] = 0
    return p


# ---- the cases -----------------------------------------------------------------------------------------------------------

def base():
    L, sp, tr = rc.base()
    return L, sp, rc.banded(tr)


def _data(L, sp, tr, steps, **kw):
    return Data(L, sp, tr, steps, rc._order(sp, tr), **kw)


def identity_case():
    L, sp, tr = base()
    v1 = tr["v1"].copy()
    v1[0, 0] = -0.0                                               # a floor corner pulled to x = -0.0
    tr["v1"] = v1
    assert np.signbit(tr["v1"][0, 0]) and tr["v1"][0, 0] == 0.0
    return _data(L, sp, tr, [("parts", two_parts(len(tr)), 2), ("pose", identity(2))])


def turn_case():
    L, sp, tr = base()
    steps = [("parts", two_parts(len(tr)), 2)]
    steps += [("pose", table(po.IDENTITY, affine(tilted(d), rc.SPHERE_C))) for d in (30.0, 60.0, 90.0)]
    return _data(L, sp, tr, steps)


def out_case():
    d = rc.data("out")
    tr = d.tr
    nw = NWALL - 2
    ext = rc.scene_extent(tr)
    room_front = float(rc.verts(tr)[:nw].reshape(-1, 3)[:, 2].min())
    c2 = np.array((0.0, 0.0, room_front - 3.0 * ext))
    rec = affine(np.eye(3) * 6.0, rc.SPHERE_C, c2 - rc.SPHERE_C)
    steps = [("parts", two_parts(len(tr), nw), 2), ("pose", table(po.IDENTITY, rec))]
    return Data(d.L, d.sp, tr, steps, rc._order(d.sp, tr), rc.OUT_EYE, rc.OUT_LOOK)


def shrink_case():
    L, sp, tr = base()
    rec = affine(np.eye(3) * 0.25, sio.CORNELL_LOOK)
    return _data(L, sp, tr, [("parts", two_parts(len(tr)), 2), ("pose", table(rec, rec))])


def shear_mirror_case():
    L, sp, tr = base()
    shear = np.array([[1.0, 0.9, 0.0], [0.0, 1.0, 0.0], [0.0, 0.4, 1.0]])
    mirror = np.diag([-1.0, 1.0, 1.0]) @ rot_y(50.0)
    assert np.linalg.det(mirror) < 0
    steps = [("parts", two_parts(len(tr)), 2),
             ("pose", table(po.IDENTITY, affine(shear, rc.SPHERE_C))),
             ("pose", table(po.IDENTITY, affine(mirror, rc.SPHERE_C, (0.2, -0.1, -0.1))))]
    return _data(L, sp, tr, steps)


def die_case():
    L, sp, tr = base()
    turned = affine(tilted(40.0), rc.SPHERE_C)
    nan1 = turned.copy(); nan1[1, 2] = NAN
    inf0 = po.IDENTITY.copy(); inf0[0, 3] = INF
    huge = affine(np.eye(3) * 1e38); huge[2, 3] = 3.3e38
    dead = po.IDENTITY.copy(); dead[2, 0] = -INF
    steps = [("parts", two_parts(len(tr)), 2),
             ("pose", table(po.IDENTITY, nan1)),
             ("pose", table(po.IDENTITY, turned)),
             ("pose", table(inf0, turned)),
             ("pose", table(po.IDENTITY, huge)),
             ("pose", table(dead, nan1)),
             ("pose", identity(2))]
    return _data(L, sp, tr, steps)


N_RANDOM = 3000


def per_triangle_case():
    d = rc.data("scramble")
    L, sp, tr = d.L, d.sp, d.tr
    assert len(tr) == NWALL + N_RANDOM
    part = np.zeros(len(tr), np.int32)
    part[NWALL:] = np.minimum(np.arange(1, N_RANDOM + 1), N_RANDOM - 1)       # 1 .. 2999, the last two share 2999
    num_parts = N_RANDOM + 1                                                  # part 3000 owns no triangle
    rng = np.random.default_rng(11)
    cen = rc.verts(tr).mean(axis=1)
    recs = np.tile(po.IDENTITY, (num_parts, 1, 1)).astype(F32)
    for k in range(1, num_parts):
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        a = np.radians(rng.uniform(40.0, 140.0))
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        c = cen[min(NWALL + k - 1, len(tr) - 1)]
        recs[k] = affine(R, c, rng.uniform(-0.08, 0.08, 3))
    return _data(L, sp, tr, [("parts", part, num_parts), ("pose", recs)])


def tiny_case(n):
    d = rc.data("tiny-%d" % n)
    a = affine(rot_z(60.0) * 0.7, shift=(0.15, 0.1, -0.2))
    b = affine(rot_y(35.0), (0, 0, 0.6), (-0.2, 0.05, 0.3))
    steps = [("parts", np.arange(n, dtype=np.int32), n), ("pose", table(*[a] * n)), ("pose", table(*[b] * n))]
    return _data(d.L, d.sp, d.tr, steps)


EDGE_COUNTS = (85, 171, 256)


def edges_case(n):
    L, sp, tr = base()
    tr = tr[:n].copy()
    rec = affine(tilted(40.0) * 4.0, rc.SPHERE_C, (0.1, -0.45, -0.5))       # large: the first 73 sphere triangles are a small cap
    return _data(L, sp, tr, [("parts", two_parts(n), 2), ("pose", table(po.IDENTITY, rec))])


def interleave_case():
    L, sp, tr = base()
    turn = table(po.IDENTITY, affine(tilted(30.0), rc.SPHERE_C))
    v = rc.verts(tr)
    v[NWALL:] += np.array((0.25, 0.0, -0.1))
    v[:NWALL, :, 0] *= 1.3
    wide = rc.with_verts(tr, v)                                          # the walls pulled apart, the sphere to the right
    v = rc.verts(tr)
    v[NWALL:] += np.array((0.1, -0.35, -0.1))
    lowered = rc.with_verts(tr, v)
    thirds = two_parts(len(tr))
    thirds[NWALL:] = 1 + (np.arange(len(tr) - NWALL) // 5) % 3           # the three colour bands, a part each
    apart = table(po.IDENTITY, affine(np.eye(3), shift=(0.0, 0.15, 0.0)), affine(rot_y(45.0), rc.SPHERE_C + np.array((0.1, -0.35, -0.1))),
                  affine(np.eye(3) * 0.5, rc.SPHERE_C))
    steps = [("parts", two_parts(len(tr)), 2), ("pose", turn), ("tris", wide), ("pose", turn), ("dverts", lowered), ("pose", turn),
             ("parts", thirds, 4), ("pose", apart)]
    return _data(L, sp, tr, steps)


DV_SOURCES = ("turn", "die-and-return", "tiny-1", "tiny-2", "tiny-3")


def device_verts_case(source):
    d = rc.data(source)
    return Data(d.L, d.sp, d.tr, [("dverts", t) for (_, _, t) in d.steps], d.order, d.eye, d.look)


def _bind(fn, *a):
    return lambda: fn(*a)


CASES = ([Case("identity", identity_case), Case("turn", turn_case), Case("out", out_case), Case("shrink", shrink_case),
          Case("shear-mirror", shear_mirror_case), Case("die-and-return", die_case), Case("per-triangle", per_triangle_case)]
         + [Case("tiny-%d" % n, _bind(tiny_case, n)) for n in (1, 2, 3)]
         + [Case("edges-%d" % n, _bind(edges_case, n)) for n in EDGE_COUNTS]
         + [Case("interleave", interleave_case)]
         + [Case("dv-" + s, _bind(device_verts_case, s)) for s in DV_SOURCES])
NAMES = [c.name for c in CASES]
CASE_BY_NAME = {c.name: c for c in CASES}
POSE_NAMES = [n for n in NAMES if not n.startswith("dv-")]
SAME_AS_BEFORE = [("identity", 1)]                                 # geometry steps that must NOT change the image
# dead triangles after a step, where the case is about them
N_DEAD = {("die-and-return", 1): 1860, ("die-and-return", 2): 0, ("die-and-return", 3): 12, ("die-and-return", 4): 1860,
          ("die-and-return", 5): 1872, ("die-and-return", 6): 0}

_DATA, _EXPECTED, _SCANS, _TREES = {}, {}, {}, {}


def data(name):
    if name not in _DATA:
        _DATA[name] = CASE_BY_NAME[name].make()
    return _DATA[name]


def camera(name):
    d = data(name)
    return sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, W, H)


def replay(d):
    """Per step (records the handle holds afterwards, rest pose, part map): the rest-pose rule, by the oracle."""
    cur, rest, part, out = d.tr, None, None, []
    for step in d.steps:
        if step[0] == "parts":
            part, rest = np.asarray(step[1], np.int64), cur
        elif step[0] == "pose":
            cur = po.pose(rest, part, step[1])
        else:                                                      # "tris", "dverts": not a pose
            cur = po.with_verts(d.tr, po.verts_of(step[1]))
            rest = cur
        out.append((cur, rest, part))
    return out


def expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = replay(data(name))
    return _EXPECTED[name]


def records(name, step):
    """(L, sp, tr) the handle holds after `step`; step -1 is the base scene."""
    d = data(name)
    return d.L, d.sp, (d.tr if step < 0 else expected(name)[step][0])


def is_geometry_step(name, step):
    return data(name).steps[step][0] != "parts"


def geometry_steps(name):
    return [s for s in range(len(data(name).steps)) if is_geometry_step(name, s)]


def pose_steps():
    return [(n, s) for n in NAMES for s in range(len(data(n).steps)) if data(n).steps[s][0] == "pose"]


def all_geometry_steps(names=None):
    return [(n, s) for n in (names or NAMES) for s in geometry_steps(n)]


def scan(oracle_mod, name, step):
    """(image, stats) of the oracle's scan of the records after `step`, once per process, read-only."""
    key = (name, step)
    if key not in _SCANS:
        d = data(name)
        if step >= 0 and d.steps[step][0] == "parts":
            _SCANS[key] = scan(oracle_mod, name, step - 1)
        else:
            L, sp, tr = records(name, step)
            img, st = oracle_mod.pt_render(L, sp, tr, camera(name), W, H, DEPTH, SPP, seed=SEED)
            img.setflags(write=False)
            _SCANS[key] = (img, st)
    return _SCANS[key]


def tree(hpt, name, step):
    """The definition's tree after `step`: hpt_bvh_refit_host from the base records (step -1: the builder's)."""
    key = (name, step)
    if key not in _TREES:
        d = data(name)
        if step < 0:
            _TREES[key] = hpt.export_bvh_host(d.L, d.sp, d.tr)
        elif d.steps[step][0] == "parts":
            _TREES[key] = tree(hpt, name, step - 1)
        else:
            _TREES[key] = hpt.refit_bvh_host(d.L, d.sp, d.tr, records(name, step)[2])
    return _TREES[key]
