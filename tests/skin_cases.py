"""Case table of the skin suite (include/hpt.h, "skinning"): a base scene and a sequence of steps on ONE live handle.  It
builds on pose_cases' and refit_cases' meshes and helpers and renders as they do: 48 x 48, depth 4, 4 spp, seed 31, the
Cornell camera.  A plain module: no GPU, no tests.

A step is one of
    ("set", corner_bone, corner_weight, num_bones)   Scene.set_skin: [n, 3, 4] int32 and float32; the rest pose is what the
                                                     scene holds now, and the parts are dropped
    ("skin", xforms)                                 Scene.skin: [num_bones, 3, 4] float32, absolute, over the rest pose
    ("parts", tri_part, num_parts), ("pose", xforms) Scene.set_parts (the skin is dropped) and Scene.pose
    ("tris", records), ("dverts", records)           Scene.update_triangles / update_vertices_device: the rest-pose rule
and expected(name)[i] are the records the handle holds after step i, by skin_oracle.  The base is pose_cases' -- 12 wall
triangles and the 1860-triangle sphere -- unless said otherwise; the walls have four zero weights unless said otherwise:

  rigid           pose_cases' `turn` table as one-hot weights of 1.0f, the hot influence in a slot that changes from corner
                  to corner: the records of hpt_scene_pose, byte for byte
  keep            a wall coordinate that is -0.0 and one that is a NaN with a payload, under zero weights; the sphere's
                  corners weighted 0.3 / 0.7 on two bones both left at identity, whatever a third, unweighted bone holds
                  (identity, then NaN); then bone 1 turns and the sphere blends
  bend            walls and a 264-triangle sphere, two bones, weights by height -- the foot rigid on bone 0 by weight 1.0f,
                  the top on bone 1 -- twisted 20, 45 and 90 degrees about the vertical axis through its centroid
  four            four active influences per sphere corner: weights summing to 2 over records scaled by 0.5 on the even
                  triangles, to 0.5 over records scaled by 2 on the odd ones
  die-and-return  a NaN bone and an infinite bone that the walls and 600 sphere triangles name with zero weight (no effect)
                  and 300 + 100 triangles with weight (dead); all bones finite (revived); a weight of 1e30 on 100
                  triangles, harmless on a bone scaled by 1e-30, overflowing once that bone is scaled by 1e10; every bone
                  at identity: the base's bytes
  rest-rule       skin, update_triangles, skin, update_vertices_device, skin: pose_cases' interleave with a skin
  swap            skin, set_parts and a pose, set_skin and a skin
  tiny-1, -2, -3  scenes of 1, 2 and 3 triangles, blended
  edges-85, -86, -171, -256
                  the first n triangles of the base: 255, 258, 513 and 768 corners in workgroups of 256
  grid-stride     174 763 triangles: 524 289 corners, one more than 2048 workgroups of 256 lanes, so the kernel's
                  grid-stride loop takes a second trip for lane 0 of workgroup 0.  Rendered by the host walk of the
                  definition's tree, not by the scan
  bones-1, -256, -257, -3001, -65536
                  both sides of the table the kernel stages in LDS, and the width of a bone index"""
import collections

import numpy as np

import pose_cases as pc
import pose_oracle as po
import refit_cases as rc
import skin_oracle as so
from path_tracing_amd import scene_io as sio

F32 = np.float32
W, H, DEPTH, SPP, SEED = rc.W, rc.H, rc.DEPTH, rc.SPP, rc.SEED
NWALL = rc.NWALL
Case = collections.namedtuple("Case", "name make")
Data = collections.namedtuple("Data", "L sp tr steps order eye look walk", defaults=(sio.CORNELL_EYE, sio.CORNELL_LOOK, False))
NAN, INF = float("nan"), float("inf")


# ---- influence tables ------------------------------------------------------------------------------------------------------

def no_weights(n):
    return np.zeros((n, 3, 4), np.int32), np.zeros((n, 3, 4), F32)


def height_weights(tr, first=NWALL):
    """Two bones: a corner of triangles [first, n) at height y has t = clamp((y - ymin) / (ymax - ymin), 0, 1) on bone 1 and
    1 - t on bone 0, in float32; every other corner four zero weights."""
    bone, weight = no_weights(len(tr))
    y = po.verts_of(tr)[first:, :, 1]
    lo, hi = F32(y.min()), F32(y.max())
    t = np.clip((y - lo) / (hi - lo), F32(0), F32(1)).astype(F32)
    bone[first:, :, 1] = 1
    weight[first:, :, 0] = F32(1) - t
    weight[first:, :, 1] = t
    return bone, weight


def scaled(rec, s):
    return (np.asarray(rec, np.float64) * s).astype(F32)


def twist(deg, centre):
    return pc.table(po.IDENTITY, pc.affine(pc.rot_y(deg), centre))


# ---- the cases -----------------------------------------------------------------------------------------------------------

def _data(L, sp, tr, steps, **kw):
    return Data(L, sp, tr, steps, rc._order(sp, tr), **kw)


def rigid_case():
    d = pc.data("turn")
    n = len(d.tr)
    part = np.asarray(d.steps[0][1])
    bone = np.ones((n, 3, 4), np.int32)                            # the cold slots name bone 1: never evaluated
    weight = np.zeros((n, 3, 4), F32)
    slot = np.arange(n * 3).reshape(n, 3) % 4
    np.put_along_axis(bone, slot[..., None], part[:, None, None], axis=-1)
    np.put_along_axis(weight, slot[..., None], F32(1), axis=-1)
    return Data(d.L, d.sp, d.tr, [("set", bone, weight, 2)] + [("skin", s[1]) for s in d.steps[1:]], d.order)


def keep_case():
    L, sp, tr = pc.base()
    v = po.verts_of(tr).view(np.uint32).copy()
    v[0, 1, 0] = 0x80000000                                        # a floor corner at x = -0.0
    v[11, 2, 1] = 0x7FC12345                                       # a wall corner that is a NaN with a payload: that wall is dead
    tr = po.with_verts(tr, v.view(F32))
    bone, weight = no_weights(len(tr))
    bone[:NWALL] = 2                                               # zero weights on the bone that turns to NaN
    bone[NWALL:, :, 1] = 1
    bone[NWALL:, :, 3] = 2
    weight[NWALL:, :, 0] = 0.3
    weight[NWALL:, :, 1] = 0.7
    nan_rec = np.full((3, 4), NAN, F32)
    steps = [("set", bone, weight, 3), ("skin", pc.identity(3)), ("skin", pc.table(po.IDENTITY, po.IDENTITY, nan_rec)),
             ("skin", pc.table(po.IDENTITY, pc.affine(pc.tilted(50.0), rc.SPHERE_C), nan_rec))]
    return _data(L, sp, tr, steps)


BEND_C, BEND_R = (-0.15, 0.25, 0.0), 0.15


def bend_mesh():
    L, sp, tr = pc.base()
    ball = sio._tris_from(sio.tessellated_sphere(BEND_C, BEND_R, 12, 12), np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), F32), (264, 1)))
    tr = np.concatenate([tr[:NWALL], ball])
    tr["id"] = np.arange(len(tr))
    return L, sp, rc.banded(tr)


def bend_case():
    L, sp, tr = bend_mesh()
    assert len(tr) == NWALL + 264
    bone, weight = height_weights(tr)
    c = po.verts_of(tr)[NWALL:].reshape(-1, 3).astype(np.float64).mean(axis=0)
    return _data(L, sp, tr, [("set", bone, weight, 2)] + [("skin", twist(a, c)) for a in (20.0, 45.0, 90.0)])


def four_case():
    L, sp, tr = pc.base()
    n = len(tr)
    bone, weight = no_weights(n)
    even = np.arange(n) % 2 == 0
    ball = np.arange(n) >= NWALL
    bone[ball & even] = np.array([1, 2, 3, 4], np.int32)
    weight[ball & even] = np.array([0.5, 0.5, 0.5, 0.5], F32)
    bone[ball & ~even] = np.array([8, 7, 6, 5], np.int32)
    weight[ball & ~even] = np.array([0.125, 0.0625, 0.25, 0.0625], F32)
    assert weight[ball & even].sum(axis=-1).max() == 2.0 and weight[ball & ~even].sum(axis=-1).max() == 0.5

    def tab(a0):
        recs = [po.IDENTITY] + [scaled(pc.affine(pc.tilted(a0 + 5.0 * k), rc.SPHERE_C), 0.5) for k in range(4)]
        recs += [scaled(pc.affine(pc.tilted(a0 + 7.0 * k), rc.SPHERE_C, (0.1, 0.0, 0.0)), 2.0) for k in range(4)]
        return pc.table(*recs)
    return _data(L, sp, tr, [("set", bone, weight, 9), ("skin", tab(25.0)), ("skin", tab(70.0))])


def die_case():
    L, sp, tr = pc.base()
    n = len(tr)
    bone, weight = no_weights(n)
    bone[:NWALL, :, 0], bone[:NWALL, :, 1] = 2, 3                  # the walls name the NaN and the infinite bone, weightless
    a, b, c, e = NWALL, NWALL + 600, NWALL + 900, NWALL + 1000
    bone[a:, :, 1] = 1
    weight[a:, :, 0] = 0.5
    weight[a:, :, 1] = 0.5
    bone[a:b, :, 2], bone[a:b, :, 3] = 2, 3                        # ... and so do 600 of the sphere
    bone[b:c, :, 0] = 2                                            # 300 follow the NaN bone
    bone[c:e, :, 3] = 3                                            # 100 the infinite bone, a little
    weight[c:e, :, 3] = 0.001
    bone[e:e + 100, :, 0] = 4                                      # 100 follow bone 4 with a weight of 1e30
    weight[e:e + 100, :, 0] = 1e30
    weight[e:e + 100, :, 1] = 0.0
    turn = pc.affine(pc.tilted(40.0), rc.SPHERE_C)
    other = pc.affine(pc.tilted(55.0), rc.SPHERE_C)
    nan2 = turn.copy(); nan2[1, 2] = NAN
    inf3 = po.IDENTITY.copy(); inf3[0, 3] = INF
    small = scaled(turn, 1e-30)
    huge = scaled(turn, 1e10)
    steps = [("set", bone, weight, 5),
             ("skin", pc.table(po.IDENTITY, turn, nan2, inf3, small)),
             ("skin", pc.table(po.IDENTITY, other, turn, other, small)),
             ("skin", pc.table(po.IDENTITY, turn, turn, turn, huge)),
             ("skin", pc.identity(5))]
    return _data(L, sp, tr, steps)


def rest_rule_case():
    d = pc.data("interleave")
    wide, lowered = d.steps[2][1], d.steps[4][1]
    bone, weight = height_weights(d.tr)
    bent = twist(60.0, rc.SPHERE_C)
    steps = [("set", bone, weight, 2), ("skin", bent), ("tris", wide), ("skin", bent), ("dverts", lowered), ("skin", bent)]
    return _data(d.L, d.sp, d.tr, steps)


def swap_case():
    L, sp, tr = pc.base()
    bone, weight = height_weights(tr)
    turn = pc.table(po.IDENTITY, pc.affine(pc.tilted(30.0), rc.SPHERE_C))
    steps = [("set", bone, weight, 2), ("skin", twist(70.0, rc.SPHERE_C)), ("parts", pc.two_parts(len(tr)), 2), ("pose", turn),
             ("set", bone, weight, 2), ("skin", twist(-70.0, rc.SPHERE_C))]
    return _data(L, sp, tr, steps)


def tiny_case(n):
    d = rc.data("tiny-%d" % n)
    bone = np.tile(np.array([0, 1, 2, 1], np.int32), (n, 3, 1))
    weight = np.tile(np.array([0.25, 0.5, 0.0, 0.25], F32), (n, 3, 1))
    weight[:, 1] = np.array([0.0, 0.0, 1.0, 0.0], F32)             # corner 1 of every triangle rigid on bone 2
    a = pc.affine(pc.rot_z(60.0) * 0.7, shift=(0.15, 0.1, -0.2))
    b = pc.affine(pc.rot_y(35.0), (0, 0, 0.6), (-0.2, 0.05, 0.3))
    steps = [("set", bone, weight, 3), ("skin", pc.table(a, b, a)), ("skin", pc.table(b, po.IDENTITY, b))]
    return _data(d.L, d.sp, d.tr, steps)


EDGE_COUNTS = (85, 86, 171, 256)


def edges_case(n):
    L, sp, tr = pc.base()
    tr = tr[:n].copy()
    bone, weight = height_weights(tr)
    rec = pc.affine(pc.tilted(40.0) * 4.0, rc.SPHERE_C, (0.1, -0.45, -0.5))     # large: the first sphere triangles are a small cap
    return _data(L, sp, tr, [("set", bone, weight, 2), ("skin", pc.table(po.IDENTITY, rec))])


N_STRIDE = 174763


def grid_stride_case():
    L, sp, tr = sio.cornell_with_sphere(177000)
    assert len(tr) > N_STRIDE
    tr = tr[:N_STRIDE].copy()
    bone, weight = height_weights(tr)
    return _data(L, sp, tr, [("set", bone, weight, 2), ("skin", twist(60.0, rc.SPHERE_C))], walk=True)


BONE_COUNTS = (1, 256, 257, 3001, 65536)


def bones_case(nb):
    L, sp, tr = pc.base()
    n = len(tr)
    bone, weight = no_weights(n)
    c = np.arange(NWALL * 3, n * 3, dtype=np.int64).reshape(n - NWALL, 3)
    bone[NWALL:, :, 0] = (c * 7) % nb
    bone[NWALL:, :, 1] = (c * 13 + 1) % nb
    bone[NWALL:, :, 2] = nb - 1
    bone[:NWALL, :, 3] = nb - 1
    weight[NWALL:] = np.array([0.5, 0.25, 0.25, 0.0], F32)
    # bone k: the tilted turn of 40 + 10 k / nb degrees about the sphere's centre, built in double and rounded once
    ang = np.radians(40.0 + 10.0 * np.arange(nb) / nb)
    ca, sa = np.cos(ang), np.sin(ang)
    z, o = np.zeros(nb), np.ones(nb)
    Rz = np.stack([np.stack([ca, -sa, z], -1), np.stack([sa, ca, z], -1), np.stack([z, z, o], -1)], 1)
    Ry = np.stack([np.stack([ca, z, sa], -1), np.stack([z, o, z], -1), np.stack([-sa, z, ca], -1)], 1)
    M = Rz @ Ry
    recs = np.zeros((nb, 3, 4))
    recs[:, :, :3] = M
    recs[:, :, 3] = rc.SPHERE_C - M @ rc.SPHERE_C
    return _data(L, sp, tr, [("set", bone, weight, nb), ("skin", recs.astype(F32))])


def _bind(fn, *a):
    return lambda: fn(*a)


CASES = ([Case("rigid", rigid_case), Case("keep", keep_case), Case("bend", bend_case), Case("four", four_case),
          Case("die-and-return", die_case), Case("rest-rule", rest_rule_case), Case("swap", swap_case)]
         + [Case("tiny-%d" % n, _bind(tiny_case, n)) for n in (1, 2, 3)]
         + [Case("edges-%d" % n, _bind(edges_case, n)) for n in EDGE_COUNTS]
         + [Case("grid-stride", grid_stride_case)]
         + [Case("bones-%d" % n, _bind(bones_case, n)) for n in BONE_COUNTS])
NAMES = [c.name for c in CASES]
CASE_BY_NAME = {c.name: c for c in CASES}
SAME_AS_BEFORE = [("keep", 1), ("keep", 2)]                        # geometry steps that must NOT change the image
# dead triangles after a step, where the case is about them (keep: the wall that holds the NaN)
N_DEAD = {("keep", 1): 1, ("keep", 3): 1, ("die-and-return", 1): 400, ("die-and-return", 2): 0, ("die-and-return", 3): 100,
          ("die-and-return", 4): 0}

_DATA, _EXPECTED, _SCANS, _TREES = {}, {}, {}, {}
_SETUP = ("set", "parts")


def data(name):
    if name not in _DATA:
        _DATA[name] = CASE_BY_NAME[name].make()
    return _DATA[name]


def camera(name):
    d = data(name)
    return sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, W, H)


def replay(d):
    """Per step (records the handle holds afterwards, rest pose, deformer): the rest-pose rule and one deformer per scene,
    by the oracles.  deformer: ("skin", bone, weight), ("parts", part) or None."""
    cur, rest, deformer, out = d.tr, None, None, []
    for step in d.steps:
        if step[0] == "set":
            deformer, rest = ("skin", step[1], step[2]), cur
        elif step[0] == "parts":
            deformer, rest = ("parts", np.asarray(step[1], np.int64)), cur
        elif step[0] == "skin":
            assert deformer[0] == "skin"
            cur = so.skin(rest, deformer[1], deformer[2], step[1])
        elif step[0] == "pose":
            assert deformer[0] == "parts"
            cur = po.pose(rest, deformer[1], step[1])
        else:                                                      # "tris", "dverts"
            cur = po.with_verts(d.tr, po.verts_of(step[1]))
            rest = cur
        out.append((cur, rest, deformer))
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
    return data(name).steps[step][0] not in _SETUP


def geometry_steps(name):
    return [s for s in range(len(data(name).steps)) if is_geometry_step(name, s)]


def skin_steps():
    return [(n, s) for n in NAMES for s in range(len(data(n).steps)) if data(n).steps[s][0] == "skin"]


def all_geometry_steps(names=None):
    return [(n, s) for n in (names or NAMES) for s in geometry_steps(n)]


def tree(hpt, name, step):
    """The definition's tree after `step`: hpt_bvh_refit_host from the base records (step -1: the builder's)."""
    key = (name, step)
    if key not in _TREES:
        d = data(name)
        if step < 0:
            _TREES[key] = hpt.export_bvh_host(d.L, d.sp, d.tr)
        elif not is_geometry_step(name, step):
            _TREES[key] = tree(hpt, name, step - 1)
        else:
            _TREES[key] = hpt.refit_bvh_host(d.L, d.sp, d.tr, records(name, step)[2])
    return _TREES[key]


def scan(oracle_mod, name, step, hpt=None):
    """(image, stats) of the oracle's render of the records after `step`, once per process, read-only: its scan of every
    primitive, or -- for a case with `walk`, whose scan would take minutes -- its walk of the definition's tree."""
    key = (name, step)
    if key not in _SCANS:
        d = data(name)
        if step >= 0 and not is_geometry_step(name, step):
            _SCANS[key] = scan(oracle_mod, name, step - 1, hpt)
        else:
            L, sp, tr = records(name, step)
            kw = {}
            if d.walk:
                assert hpt is not None, "a walked case needs the library for its tree"
                kw["bvh"] = tree(hpt, name, step)
            img, st = oracle_mod.pt_render(L, sp, tr, camera(name), W, H, DEPTH, SPP, seed=SEED, **kw)
            img.setflags(write=False)
            _SCANS[key] = (img, st)
    return _SCANS[key]
