"""Case table of the morph suite (include/hpt.h, "morph targets"): a base scene and a sequence of steps on ONE live handle.
It builds on skin_cases', pose_cases' and refit_cases' meshes and helpers and renders as they do: 48 x 48, depth 4, 4 spp,
seed 31, the Cornell camera.  A plain module: no GPU, no tests.

A step is one of
    ("morphs", target_begin, entry_corner, entry_delta)   Scene.set_morphs: the rest pose is what the scene holds now
    ("morph", weights)                                    Scene.morph: one float32 per target, absolute
    ("parts", tri_part, num_parts), ("pose", xforms)      Scene.set_parts and Scene.pose
    ("set", corner_bone, corner_weight, num_bones), ("skin", xforms)      Scene.set_skin and Scene.skin
    ("tris", records), ("dverts", records)                Scene.update_triangles / update_vertices_device
and expected(name)[i] is the State after step i, by morph_oracle, pose_oracle and skin_oracle: morph first, then the
deformer.  The mesh is skin_cases' bend_mesh -- 12 wall triangles and a 264-triangle sphere -- unless said otherwise:

  zero            a wall coordinate that is -0.0 and one that is a NaN with a payload, both named by a target; all weights
                  +0, then -0 and +0 mixed: not a bit moves; then the sphere's target at 1 with the walls' at -0
  exact           one target at weight 1 whose deltas are minus half the rest vertex: rest + d is exact, half the vertex
  order           three targets on every sphere corner, +64, -64 and a small offset along x, at weight 1: the float sum
                  depends on the order
  contract        a radial bulge at weight 0.3 (w * d is inexact, so a fused multiply-add rounds differently), then a
                  denormal weight on a target of deltas near 1e37, then a negative weight
  die-and-return  a target of NaN deltas on 60 triangles and two of the floor at weight 0 (no effect), at 1 (dead) and back (revived); an
                  infinite weight and a 1e30 weight on a target of 1e10 deltas over 40 triangles (dead); all zero: the base
  sparse          four targets: an empty one, one whose only entry is the first corner, one whose only entry is the last
                  corner, an empty one
  no-entries      two targets without a single entry, at weights 1 and 2: not a bit moves
  all-4096        one triangle whose corner 1 is named by every one of 4096 targets, weights of both signs
  one-each        the base of pose_cases (1872 triangles): 4096 targets with one entry each, on 4096 corners of the sphere
  tiny-1, -2, -3  scenes of 1, 2 and 3 triangles, two dense targets
  edges-85, -86   the first n triangles of pose_cases' base: 255 and 258 corners in workgroups of 256
  grid-stride     174 763 triangles: 524 289 corners, one more than 2048 workgroups of 256 lanes, so the kernel's
                  grid-stride loop takes a second trip for lane 0 of workgroup 0; one target on every tenth corner.
                  Rendered by the host walk of the definition's tree, not by the scan
  with-parts      set_morphs, set_parts, then morph, pose, morph, pose: every step the deformer's last table over M
  with-skin       the same with a skin
  recapture       a morph, then set_parts: the morphed geometry is the rest pose and the weights are zero again
  tris-between    morph, update_triangles, morph; then update_vertices_device and a morph
  swap            morphs and parts, a pose and a morph; set_skin replaces the parts and keeps the morphs
  twice           set_morphs, a morph, set_morphs with other targets over the morphed geometry, a morph"""
import collections

import numpy as np

import morph_oracle as mo
import pose_cases as pc
import pose_oracle as po
import refit_cases as rc
import skin_cases as sc
import skin_oracle as so
from path_tracing_amd import scene_io as sio

F32, U32 = np.float32, np.uint32
W, H, DEPTH, SPP, SEED = rc.W, rc.H, rc.DEPTH, rc.SPP, rc.SEED
NWALL = rc.NWALL
MAX_TARGETS = 4096
Case = collections.namedtuple("Case", "name make")
Data = collections.namedtuple("Data", "L sp tr steps order eye look walk", defaults=(sio.CORNELL_EYE, sio.CORNELL_LOOK, False))
# after a step: the records the handle holds, the rest pose R, the morphed rest pose M, the deformer (("parts", part),
# ("skin", bone, weight) or None) with its last table (None: identity), the targets (tb, ec, ed) or None, the last weights
State = collections.namedtuple("State", "tr rest morphed deformer table targets weights")
NAN, INF = float("nan"), float("inf")
BEND_C = np.array(sc.BEND_C, np.float64)


# ---- targets ---------------------------------------------------------------------------------------------------------------

def targets(*each):
    """(target_begin, entry_corner, entry_delta) from one (corners, deltas) pair per target."""
    tb = np.zeros(len(each) + 1, np.int32)
    tb[1:] = np.cumsum([len(c) for c, _ in each])
    ec = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in each] + [np.zeros(0, np.int32)])
    ed = np.concatenate([np.asarray(d, F32).reshape(-1, 3) for _, d in each] + [np.zeros((0, 3), F32)])
    return tb, ec.astype(np.int32), np.ascontiguousarray(ed, F32)


EMPTY = (np.zeros(0, np.int32), np.zeros((0, 3), F32))


def corners_of(first, last):
    return np.arange(first * 3, last * 3, dtype=np.int32)


def radial(tr, first, last, centre, scale):
    """(corners, deltas): every corner of triangles [first, last) pushed away from `centre` by `scale` times its offset."""
    v = po.verts_of(tr)[first:last].reshape(-1, 3).astype(np.float64)
    return corners_of(first, last), ((v - np.asarray(centre, np.float64)) * scale).astype(F32)


def lift(tr, first, last, scale):
    """(corners, deltas): every corner of triangles [first, last) lifted by `scale` times its height in the range."""
    y = po.verts_of(tr)[first:last].reshape(-1, 3)[:, 1].astype(np.float64)
    h = (y - y.min()) / max(y.max() - y.min(), 1e-30)
    d = np.zeros((len(y), 3))
    d[:, 1] = h * scale
    return corners_of(first, last), d.astype(F32)


def const(first, last, delta):
    c = corners_of(first, last)
    return c, np.tile(np.asarray(delta, F32), (len(c), 1))


def w(*values):
    return np.array(values, F32)


def two_shapes(tr, first=NWALL, centre=BEND_C):
    """The pair most cases use: a radial bulge of a half and a lift of 0.1 on the mesh's triangles [first, n)."""
    return targets(radial(tr, first, len(tr), centre, 0.5), lift(tr, first, len(tr), 0.1))


# ---- the cases -----------------------------------------------------------------------------------------------------------

def _data(L, sp, tr, steps, **kw):
    return Data(L, sp, tr, steps, rc._order(sp, tr), **kw)


def zero_case():
    L, sp, tr = sc.bend_mesh()
    v = po.verts_of(tr).view(U32).copy()
    v[0, 1, 0] = 0x80000000                                        # a floor corner at x = -0.0
    v[11, 2, 1] = 0x7FC12345                                       # a wall corner that is a NaN with a payload: that wall is dead
    tr = po.with_verts(tr, v.view(F32))
    n = len(tr)
    t = targets(radial(tr, NWALL, n, BEND_C, 0.5), const(0, NWALL, (0.25, NAN, -0.5)), lift(tr, 0, n, 0.1))
    neg0 = np.array([0x80000000], U32).view(F32)[0]
    steps = [("morphs",) + t, ("morph", w(0.0, 0.0, 0.0)), ("morph", w(neg0, 0.0, neg0)), ("morph", w(1.0, neg0, 0.0))]
    return _data(L, sp, tr, steps)


def exact_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    c = corners_of(NWALL, n)
    rest = po.verts_of(tr)[NWALL:].reshape(-1, 3)
    d = (rest * F32(-0.5)).astype(F32)                             # exact: a power of two
    t = targets((c, d))
    got = mo.morph_verts(po.verts_of(tr), *t, w(1.0))[NWALL:].reshape(-1, 3)
    assert np.array_equal(got.astype(np.float64), rest.astype(np.float64) * 0.5)
    return _data(L, sp, tr, [("morphs",) + t, ("morph", w(1.0))])


def order_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    t = targets(const(NWALL, n, (64.0, 0.0, 0.0)), const(NWALL, n, (-64.0, 0.0, 0.0)), const(NWALL, n, (0.0123, 0.0, 0.0)))
    return _data(L, sp, tr, [("morphs",) + t, ("morph", w(1.0, 1.0, 1.0))])


def contract_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    far_c, far_d = radial(tr, NWALL, n, BEND_C, 1.0)
    far_d = (far_d.astype(np.float64) / 0.15 * 1e37).astype(F32)   # unit offsets times 1e37
    t = targets(radial(tr, NWALL, n, BEND_C, 0.37), (far_c, far_d))
    tiny = F32(5e-39)
    assert 0 < tiny < np.finfo(F32).tiny                           # a denormal weight: active, and 5e-39 * 1e37 = 0.05
    steps = [("morphs",) + t, ("morph", w(0.3, 0.0)), ("morph", w(0.0, tiny)), ("morph", w(-0.45, 0.0))]
    return _data(L, sp, tr, steps)


def die_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    a, b, c = NWALL + 100, NWALL + 160, NWALL + 200
    nan_d = const(a, b, (NAN, 0.0, INF))
    # the NaN target names the walls' first corners as well: under a zero weight they are never looked at
    nan_t = (np.concatenate([corners_of(0, 2), nan_d[0]]), np.concatenate([np.full((6, 3), NAN, F32), nan_d[1]]))
    big = const(b, c, (1e10, 0.0, 0.0))
    t = targets(radial(tr, NWALL, n, BEND_C, 0.5), nan_t, big)
    steps = [("morphs",) + t, ("morph", w(0.5, 0.0, 0.0)), ("morph", w(0.5, 1.0, 0.0)), ("morph", w(0.25, 0.0, 0.0)),
             ("morph", w(0.5, 0.0, INF)), ("morph", w(0.5, 0.0, 1e-12)), ("morph", w(0.5, 0.0, 1e30)), ("morph", w(0.0, 0.0, 0.0))]
    return _data(L, sp, tr, steps)


def sparse_case():
    L, sp, tr = sc.bend_mesh()
    last = len(tr) * 3 - 1
    t = targets(EMPTY, ([0], [(0.0, 0.2, 0.0)]), ([last], [(0.1, 0.1, 0.0)]), EMPTY)
    steps = [("morphs",) + t, ("morph", w(3.0, 1.0, 0.0, 3.0)), ("morph", w(3.0, 0.0, 1.0, 3.0)), ("morph", w(0.0, 0.5, 2.0, 0.0))]
    return _data(L, sp, tr, steps)


def no_entries_case():
    L, sp, tr = sc.bend_mesh()
    return _data(L, sp, tr, [("morphs",) + targets(EMPTY, EMPTY), ("morph", w(1.0, 2.0))])


def all_targets_case():
    d = rc.data("tiny-1")
    k = np.arange(MAX_TARGETS)
    delta = np.zeros((MAX_TARGETS, 3))
    delta[:, 0] = 0.01 * np.sin(k * 0.37)
    delta[:, 1] = 0.0003 * (1 + k % 7)
    delta[:, 2] = -0.02 * np.cos(k * 0.11)
    t = targets(*[([1], [delta[i]]) for i in range(MAX_TARGETS)])
    w1 = (np.where(k % 3 == 0, -1.0, 1.0) * (0.25 + (k % 5) * 0.125)).astype(F32)
    w2 = w1[::-1].copy()
    w2[::2] = 0.0                                                  # every other target inactive
    return _data(d.L, d.sp, d.tr, [("morphs",) + t, ("morph", w1), ("morph", w2)])


def one_each_case():
    L, sp, tr = pc.base()
    k = np.arange(MAX_TARGETS)
    corner = NWALL * 3 + k
    v = po.verts_of(tr).reshape(-1, 3)[corner].astype(np.float64)
    delta = ((v - rc.SPHERE_C) * 0.5).astype(F32)
    t = targets(*[([corner[i]], [delta[i]]) for i in range(MAX_TARGETS)])
    w1 = (0.5 + (k % 4) * 0.25).astype(F32)
    w1[k % 9 == 0] = 0.0
    return _data(L, sp, tr, [("morphs",) + t, ("morph", w1)])


def tiny_case(n):
    d = rc.data("tiny-%d" % n)
    c = corners_of(0, n)
    d0 = np.tile(np.array([(0.1, 0.0, 0.05), (0.0, 0.15, 0.0), (-0.1, 0.05, 0.0)], F32), (n, 1))
    d1 = np.tile(np.array([(0.0, -0.1, 0.0), (0.05, 0.0, -0.1), (0.0, 0.0, 0.2)], F32), (n, 1))
    t = targets((c, d0), (c, d1))
    return _data(d.L, d.sp, d.tr, [("morphs",) + t, ("morph", w(0.7, 0.3)), ("morph", w(-0.5, 1.25))])


EDGE_COUNTS = (85, 86)


def edges_case(n):
    L, sp, tr = pc.base()
    tr = tr[:n].copy()
    # the last corners on both sides of the workgroup's edge get a target of their own
    t = targets(radial(tr, NWALL, n, rc.SPHERE_C, 3.0), const(n - 2, n, (0.0, -0.3, -0.2)))
    return _data(L, sp, tr, [("morphs",) + t, ("morph", w(1.0, 1.0))])


N_STRIDE = sc.N_STRIDE


def grid_stride_case():
    L, sp, tr = sio.cornell_with_sphere(177000)
    assert len(tr) > N_STRIDE
    tr = tr[:N_STRIDE].copy()
    c = np.arange(NWALL * 3, N_STRIDE * 3, 10, dtype=np.int32)
    c = np.unique(np.concatenate([c, np.array([N_STRIDE * 3 - 1], np.int32)]))      # ... and the second trip's corner
    v = po.verts_of(tr).reshape(-1, 3)[c].astype(np.float64)
    t = targets((c, ((v - rc.SPHERE_C) * 0.4).astype(F32)))
    return _data(L, sp, tr, [("morphs",) + t, ("morph", w(1.0))], walk=True)


def with_parts_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    turn = lambda deg: pc.table(po.IDENTITY, pc.affine(pc.tilted(deg), BEND_C))
    steps = [("morphs",) + two_shapes(tr), ("parts", pc.two_parts(n), 2), ("morph", w(0.8, 0.0)), ("pose", turn(30.0)),
             ("morph", w(0.2, 1.0)), ("pose", turn(75.0))]
    return _data(L, sp, tr, steps)


def with_skin_case():
    L, sp, tr = sc.bend_mesh()
    bone, weight = sc.height_weights(tr)
    steps = [("set", bone, weight, 2), ("morphs",) + two_shapes(tr), ("morph", w(0.8, 0.0)), ("skin", sc.twist(40.0, BEND_C)),
             ("morph", w(0.2, 1.0)), ("skin", sc.twist(90.0, BEND_C))]
    return _data(L, sp, tr, steps)


def recapture_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    turn = pc.table(po.IDENTITY, pc.affine(pc.tilted(50.0), BEND_C))
    steps = [("morphs",) + two_shapes(tr), ("morph", w(0.6, 0.5)), ("parts", pc.two_parts(n), 2), ("pose", turn), ("morph", w(0.6, 0.5))]
    return _data(L, sp, tr, steps)


def tris_between_case():
    L, sp, tr = sc.bend_mesh()
    v = po.verts_of(tr).astype(np.float64)
    wide = v.copy(); wide[NWALL:] = (wide[NWALL:] - BEND_C) * 1.4 + BEND_C
    low = v.copy(); low[NWALL:, :, 1] -= 0.08
    wide, low = po.with_verts(tr, wide.astype(F32)), po.with_verts(tr, low.astype(F32))
    steps = [("morphs",) + two_shapes(tr), ("morph", w(0.5, 0.5)), ("tris", wide), ("morph", w(0.5, 0.5)), ("dverts", low), ("morph", w(-0.3, 1.0))]
    return _data(L, sp, tr, steps)


def swap_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    bone, weight = sc.height_weights(tr)
    turn = pc.table(po.IDENTITY, pc.affine(pc.tilted(30.0), BEND_C))
    steps = [("morphs",) + two_shapes(tr), ("parts", pc.two_parts(n), 2), ("pose", turn), ("morph", w(0.7, 0.2)),
             ("set", bone, weight, 2), ("morph", w(0.0, 1.0)), ("skin", sc.twist(-70.0, BEND_C))]
    return _data(L, sp, tr, steps)


def twice_case():
    L, sp, tr = sc.bend_mesh()
    n = len(tr)
    other = targets(const(NWALL, NWALL + 132, (0.0, 0.0, 0.2)), EMPTY, lift(tr, NWALL + 100, n, -0.1))
    steps = [("morphs",) + two_shapes(tr), ("morph", w(0.5, 0.0)), ("morphs",) + other, ("morph", w(1.0, 5.0, 1.0))]
    return _data(L, sp, tr, steps)


def _bind(fn, *a):
    return lambda: fn(*a)


CASES = ([Case("zero", zero_case), Case("exact", exact_case), Case("order", order_case), Case("contract", contract_case),
          Case("die-and-return", die_case), Case("sparse", sparse_case), Case("no-entries", no_entries_case),
          Case("all-4096", all_targets_case), Case("one-each", one_each_case)]
         + [Case("tiny-%d" % n, _bind(tiny_case, n)) for n in (1, 2, 3)]
         + [Case("edges-%d" % n, _bind(edges_case, n)) for n in EDGE_COUNTS]
         + [Case("grid-stride", grid_stride_case)]
         + [Case("with-parts", with_parts_case), Case("with-skin", with_skin_case), Case("recapture", recapture_case),
            Case("tris-between", tris_between_case), Case("swap", swap_case), Case("twice", twice_case)])
NAMES = [c.name for c in CASES]
CASE_BY_NAME = {c.name: c for c in CASES}
# geometry steps that must NOT change the image: they leave the bytes the handle held
SAME_AS_BEFORE = [("zero", 1), ("zero", 2), ("no-entries", 1)]
# dead triangles after a step, where the case is about them (zero: the wall that holds the NaN)
N_DEAD = {("zero", 1): 1, ("zero", 3): 1, ("die-and-return", 1): 0, ("die-and-return", 2): 62, ("die-and-return", 3): 0,
          ("die-and-return", 4): 40, ("die-and-return", 5): 0, ("die-and-return", 6): 40, ("die-and-return", 7): 0}

_DATA, _EXPECTED, _SCANS, _TREES = {}, {}, {}, {}
_SETUP = ("morphs", "parts", "set")


def data(name):
    if name not in _DATA:
        _DATA[name] = CASE_BY_NAME[name].make()
    return _DATA[name]


def camera(name):
    d = data(name)
    return sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, W, H)


def deform(morphed, deformer, table):
    """The deformer's stage: its own definition with M as the rest pose; no deformer, or a table never given: M."""
    if deformer is None or table is None:
        return morphed
    if deformer[0] == "parts":
        return po.pose(morphed, deformer[1], table)
    return so.skin(morphed, deformer[1], deformer[2], table)


def replay(d, **kw):
    """One State per step.  Every step that captures a rest pose -- the three set calls, update_triangles and
    update_vertices_device -- leaves R = M = the geometry, the weights at zero and the table at identity; set_parts and
    set_skin replace each other and keep the targets.  kw goes to morph_oracle (fuse, descending)."""
    cur, rest, morphed, deformer, table, tg, wts, out = d.tr, None, None, None, None, None, None, []
    for step in d.steps:
        kind = step[0]
        if kind in ("morphs", "parts", "set", "tris", "dverts"):
            if kind == "morphs":
                tg = tuple(step[1:])
            elif kind == "parts":
                deformer = ("parts", np.asarray(step[1], np.int64))
            elif kind == "set":
                deformer = ("skin", step[1], step[2])
            else:
                cur = po.with_verts(d.tr, po.verts_of(step[1]))
            rest = morphed = cur
            table = None
            wts = None if tg is None else np.zeros(len(tg[0]) - 1, F32)
        elif kind == "morph":
            wts = np.asarray(step[1], F32)
            morphed = mo.morph(rest, *tg, wts, **kw)
            cur = deform(morphed, deformer, table)
        else:                                                      # "pose", "skin"
            assert deformer[0] == ("parts" if kind == "pose" else "skin")
            table = step[1]
            cur = deform(morphed, deformer, table)
        out.append(State(cur, rest, morphed, deformer, table, tg, wts))
    return out


def host_chain(hpt, st):
    """The records of a State by the library's host definitions alone: hpt_morph_host, then hpt_pose_host or hpt_skin_host."""
    m = st.rest if st.targets is None else hpt.morph_host(st.rest, *st.targets, st.weights)
    if st.deformer is None or st.table is None:
        return m
    if st.deformer[0] == "parts":
        return hpt.pose_host(m, st.deformer[1].astype(np.int32), st.table)
    return hpt.skin_host(m, st.deformer[1], st.deformer[2], st.table)


def expected(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = replay(data(name))
    return _EXPECTED[name]


def records(name, step):
    """(L, sp, tr) the handle holds after `step`; step -1 is the base scene."""
    d = data(name)
    return d.L, d.sp, (d.tr if step < 0 else expected(name)[step].tr)


def is_geometry_step(name, step):
    return data(name).steps[step][0] not in _SETUP


def geometry_steps(name):
    return [s for s in range(len(data(name).steps)) if is_geometry_step(name, s)]


def morph_steps(names=None):
    return [(n, s) for n in (names or NAMES) for s in range(len(data(n).steps)) if data(n).steps[s][0] == "morph"]


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
