"""The case table of the motion tests (include/hpt.h, "motion"): the previous geometry a scene remembers, the motion guide
and the history advance that follows it.  A plain module: no GPU, no tests.

Guide cases are rendered scenes: the closed Cornell room (12 triangles, a mirror back wall), a 264-triangle tessellated
sphere (the "mesh") and one rough sphere record.  A case is a list of steps on ONE live handle -- ("tris", records),
("rounds", lights, spheres) or ("keep",) -- after which the five guide images are rendered; replay() gives the current and
the previous records the handle then holds, which is what the oracle is given.

History cases use analytic guides as history_cases.py does (its closed room seen through the pixel centres), with a
sphere that moves between frames: prev_position is the wall point itself (the same bits) and, on the sphere,
c' + (X - c) * (r' / r) in float.  `room=False` leaves the sphere alone in front of nothing: sky."""
import collections

import numpy as np

from path_tracing_amd import scene_io as sio
from path_tracing_amd.layouts import SPHERE

import history_cases as hc
import refit_cases as rc

f32 = np.float32
NWALL = 12
MESH_C = np.array((-0.15, 0.2, 0.45), np.float64)
SEED = (0x9E3779B97F4A7C15 ^ 77)            # a 64-bit seed
NAN = float("nan")

# ---- guide cases ---------------------------------------------------------------------------------------------------

GuideCase = collections.namedtuple("GuideCase", "name base steps W H spp offset tile", defaults=(50, 37, 4, 3, 8))


def rough_sphere(glass=False):
    sp = np.zeros(2 if glass else 1, SPHERE)
    sp[0]["center"] = (0.25, -0.3, 0.2); sp[0]["r"] = 0.15
    sio._fill_mtl(sp[0], (0.3, 0.5, 0.9, 1.0, 0.0, 0.0))
    if glass:       # between the eye and the mesh
        sp[1]["center"] = (-0.1, 0.14, -0.2); sp[1]["r"] = 0.12
        sio._fill_mtl(sp[1], (1.0, 1.0, 1.0, 0.0, 0.0, 1.5))
        sp[1]["id"] = 1
    return sp


def base(glass=False, slivers=False):
    L, _, tr = sio.cornell_with_sphere(300)
    assert len(tr) == NWALL + 264
    if slivers:
        tr = np.concatenate([tr, sliver_tris()])
        tr["id"] = np.arange(len(tr))
    return L, rough_sphere(glass), tr


def sliver_tris(n=8):
    """Thin triangles in front of the eye with e1 = (1/2, 0, 0) and e2 = (1/2, 2^-14, 0), every subtraction exact:
    d00 = d01 = 1/4 and d11 = 1/4 + 2^-28 rounds to 1/4, so den = 1/16 - 1/16 = 0 although the triangle has area."""
    rows = []
    for k in range(n):
        y = k / 32.0 - 0.125
        rows.append((-0.25, y, -0.5, 0.25, y, -0.5, 0.25, y + 2.0 ** -14, -0.5))
    return sio._tris_from(rows, [(0.9, 0.1, 0.9, 1.0, 0.0, 0.0)] * n)


MESH = slice(NWALL, NWALL + 264)


def moved_mesh(tr, fn):
    return rc.with_verts(tr, fn(rc.verts(tr)[MESH]), MESH)


def turn(deg):
    return lambda v: rc.rotate_y(v, MESH_C, deg)


def _guide_cases():
    out = []
    L, sp, tr = base()
    add = lambda name, steps, b=(False, False), **kw: out.append(GuideCase(name, b, steps, **kw))
    add("none", [])
    add("translation", [("tris", moved_mesh(tr, lambda v: v + np.array((0.125, -0.0625, -0.25))))])
    add("turn_5", [("tris", moved_mesh(tr, turn(5.0)))])
    add("turn_40", [("tris", moved_mesh(tr, turn(40.0)))], spp=1)
    add("scale", [("tris", moved_mesh(tr, lambda v: (v - MESH_C) * np.array((1.4, 0.7, 1.1)) + MESH_C))])
    cen = rc.verts(tr)[MESH].mean(axis=1)
    k = NWALL + int(np.argmin(((cen - (MESH_C + np.array((0.0, 0.0, -0.18)))) ** 2).sum(-1)))      # the one that faces the eye
    one = slice(k, k + 1)
    add("one_triangle", [("tris", rc.with_verts(tr, rc.verts(tr)[one] + np.array((0.0, 0.0, -0.05)), one))])
    # dead in G' and alive in G: the first update kills a few mesh triangles, keep, the second brings them back
    some = [NWALL + k for k in range(90, 130, 4)]
    dead = tr.copy()
    v0 = dead["v0"].copy(); v0[some, 1] = NAN; dead["v0"] = v0
    add("dead_then_alive", [("tris", dead), ("keep",), ("tris", tr.copy())])
    add("alive_then_dead", [("tris", dead)])
    sp_c, sp_r, sp_b = sp.copy(), sp.copy(), sp.copy()
    sp_c[0]["center"] = (0.2, -0.25, 0.1)
    sp_r[0]["r"] = 0.2
    sp_b[0]["center"] = (0.3, -0.2, 0.3); sp_b[0]["r"] = 0.1
    add("sphere_moved", [("rounds", L, sp_c)])
    add("sphere_radius", [("rounds", L, sp_r)])
    add("sphere_both", [("rounds", L, sp_b), ("tris", moved_mesh(tr, turn(5.0)))])
    trg = base(glass=True)[2]
    add("glass_in_front", [("tris", moved_mesh(trg, turn(5.0)))], b=(True, False))
    a, b2 = moved_mesh(tr, turn(5.0)), moved_mesh(tr, turn(10.0))
    add("keep_between_updates", [("tris", a), ("keep",), ("tris", b2)])
    add("two_updates_no_keep", [("tris", a), ("tris", b2)])
    add("keep_after_update", [("tris", a), ("keep",)])
    trs = base(slivers=True)[2]
    moved = rc.with_verts(trs, rc.verts(trs)[-8:] + np.array((0.0, 0.0078125, 0.0)), slice(len(trs) - 8, None))
    add("sliver", [("tris", moved)], b=(False, True), W=64, H=48, tile=32)
    add("one_pixel", [("tris", moved_mesh(tr, turn(5.0)))], W=1, H=1)
    add("tile_32", [("tris", moved_mesh(tr, turn(5.0))), ("rounds", L, sp_c)], W=64, H=48, tile=32, spp=1)
    return out


GUIDE_CASES = _guide_cases()
GUIDE_BY_NAME = {c.name: c for c in GUIDE_CASES}


def guide_camera(case):
    return sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, case.W, case.H)


def replay(case):
    """((L, sp, tr) current, (sp, tr) previous, has_motion) after the case's steps."""
    L, sp, tr = base(*case.base)
    psp, ptr, motion = sp, tr, False
    for step in case.steps:
        if step[0] == "tris":
            tr, motion = step[1], True
        elif step[0] == "rounds":
            L, sp, motion = step[1], step[2], True
        else:
            psp, ptr, motion = sp, tr, False
    return (L, sp, tr), (psp, ptr), motion


def apply_steps(scene, case):
    for step in case.steps:
        if step[0] == "tris":
            scene.update_triangles(step[1])
        elif step[0] == "rounds":
            scene.update_rounds(step[1], step[2])
        else:
            scene.keep_previous()


_ORACLE = {}


def guide_oracle(mlib, name):
    """The oracle's five images of a guide case, once per process, read-only."""
    import motion_oracle
    if name not in _ORACLE:
        case = GUIDE_BY_NAME[name]
        (L, sp, tr), (psp, ptr), _ = replay(case)
        g, hp = motion_oracle.render(mlib, L, sp, tr, psp, ptr, guide_camera(case), case.W, case.H, case.spp, seed=SEED, sample_offset=case.offset)
        for v in g.values():
            v.setflags(write=False)
        _ORACLE[name] = (g, hp)
    return _ORACLE[name]


# ---- history cases -------------------------------------------------------------------------------------------------

SPH_C = np.array((0.3, -0.2, 1.2))
SPH_R = 0.5


def guides(cam, W, H, c=SPH_C, r=SPH_R, c_prev=None, r_prev=None, room=True):
    """history_cases.guides with the sphere at (c, r), plus prev_position against the sphere at (c_prev, r_prev)."""
    c = np.asarray(c, np.float64)
    old = hc.SPHERE_C, hc.SPHERE_R
    hc.SPHERE_C, hc.SPHERE_R = c, float(r)
    try:
        g = hc.guides(cam, W, H, sphere=True)
    finally:
        hc.SPHERE_C, hc.SPHERE_R = old
    pos = g["position"]
    with np.errstate(invalid="ignore"):
        d = pos.astype(np.float64) - c
        on_sphere = np.abs(np.sqrt((d * d).sum(-1)) - r) < 1e-4
    if not room:
        g["coverage"] = np.where(on_sphere, g["coverage"], f32(0)).astype(f32)
        g["position"] = np.where(on_sphere[..., None], pos, f32(0)).astype(f32)
        g["normal"] = np.where(on_sphere[..., None], g["normal"], f32(0)).astype(f32)
        pos = g["position"]
    prev = pos.copy()
    cp = c if c_prev is None else np.asarray(c_prev, np.float64)
    rp = r if r_prev is None else r_prev
    if not (np.array_equal(cp, c) and rp == r):
        cf, cpf = c.astype(f32), cp.astype(f32)
        k = f32(rp) / f32(r)
        moved = cpf + (pos - cf) * k
        prev = np.where(on_sphere[..., None], moved, pos).astype(f32)
    g["prev_position"] = prev
    return g


def _adv(cam, g, seed, params=None, in_place=False, motion=True):
    return ("advance", dict(camera=cam, guides=g, frame=hc.frame(g, seed), params=params or {}, in_place=in_place, motion=motion))


def sphere_path(k):
    """The sphere's centre in frame k: it crosses the view from left to right."""
    return SPH_C + np.array((0.12 * k - 0.3, 0.02 * k, 0.0))


def _moving(W, H, cams, params=None, seed=0, room=True, start=0):
    out = []
    for k, cam in enumerate(cams):
        c, cp = sphere_path(start + k), sphere_path(start + k - 1) if k else sphere_path(start + k)
        out.append(_adv(cam, guides(cam, W, H, c=c, c_prev=cp, room=room), 100 * seed + k, params))
    return out


def _poisoned(W, H):
    """A still camera with a moving sphere whose motion guide holds, in a few pixels of the third frame: NaN, +-inf, a
    point behind the previous camera, points off every border, and -0.0 where the position is 0.0."""
    cam = hc.camera(W, H)
    steps = _moving(W, H, [cam] * 4, seed=5)
    steps[1][1]["guides"]["coverage"][5, 5] = 0.0               # a wall pixel whose previous record has no coverage in frame 2 (3')
    g = steps[2][1]["guides"]
    p = g["prev_position"]
    p[0, 0] = (NAN, 0.0, 0.0); p[0, 1] = (np.inf, 1.0, 1.0); p[0, 2] = (0.0, -np.inf, 1.0); p[0, 3] = (NAN, NAN, NAN)
    p[1, 0] = (0.0, 0.0, -5.0)                                  # behind the camera
    p[1, 1] = (-40.0, 0.0, 2.5); p[1, 2] = (40.0, 0.0, 2.5); p[1, 3] = (0.0, 40.0, 2.5); p[1, 4] = (0.0, -40.0, 2.5)
    # "same" broken by the sign of zero: the back wall's pixel whose x is made +0.0 against -0.0
    g["position"][H - 1, 0, 0] = 0.0
    p[H - 1, 0] = g["position"][H - 1, 0]; p[H - 1, 0, 0] = -0.0
    return steps


def _history_cases():
    out = {}
    for W, H in [(1, 1), (3, 2), (131, 2), (65, 5)]:
        cams = [hc.camera(W, H)] * 3 + [hc.orbit(W, H, 3.0), hc.orbit(W, H, 6.0)]
        out["size_%dx%d" % (W, H)] = _moving(W, H, cams, seed=W + H)
    W, H = hc.MOTION_SIZE
    still = hc.camera(W, H)
    out["still_cover_uncover"] = _moving(W, H, [still] * 6, seed=1)
    out["moving_camera"] = _moving(W, H, [still, still] + [hc.orbit(W, H, 2.0 * k) for k in range(1, 5)], seed=2)
    out["sky_and_object"] = _moving(W, H, [still] * 6, seed=3, room=False)
    out["sky_and_object_moving_camera"] = _moving(W, H, [still, still, hc.orbit(W, H, 2.0), hc.orbit(W, H, 2.0), hc.orbit(W, H, 4.0)], seed=4, room=False)
    out["poisoned"] = _poisoned(W, H)
    for name, prm in (("plane_off", dict(plane_tolerance=-1.0)), ("normal_off", dict(normal_min=-2.0)),
                      ("both_off", dict(plane_tolerance=-1.0, normal_min=-2.0)), ("tight", dict(plane_tolerance=1e-4, normal_min=0.999))):
        out["switch_" + name] = _moving(W, H, [still] * 3 + [hc.orbit(W, H, 3.0)], prm, seed=6)
    for mh in (1.0, 4.0):
        out["max_history_%g" % mh] = _moving(23, 5, [hc.camera(23, 5)] * 7 + [hc.orbit(23, 5, 1.0)], dict(max_history=mh), seed=int(mh))
    out["in_place"] = [(op, dict(a, in_place=True)) for op, a in _moving(W, H, [still] * 3 + [hc.orbit(W, H, 3.0)], seed=7)]
    seq = _moving(W, H, [still] * 5, seed=8)
    out["reset_mid_sequence"] = seq[:3] + [("reset",)] + seq[3:]
    # a plain advance before and after a motion advance on one object
    seq = _moving(W, H, [still, still, still, hc.orbit(W, H, 3.0), hc.orbit(W, H, 3.0)], seed=9)
    out["plain_between"] = [(op, dict(a, motion=k in (1, 3))) for k, (op, a) in enumerate(seq)]
    # no geometry motion at all: the motion advance must equal the plain one in mean, length and counts
    out["static_scene"] = [_adv(cam, guides(cam, W, H), 900 + k) for k, cam in enumerate([still, still, hc.orbit(W, H, 4.0), hc.orbit(W, H, 4.0), hc.orbit(W, H, 8.0)])]
    return out


HISTORY_CASES = _history_cases()


def run_history_oracle(steps, W, H, motion=True):
    """Per advance: dict(mean, length, q, kept, restarted, frames, variance, branches).  motion=False: every advance plain."""
    import motion_history_oracle as mho
    h = mho.MotionHistory(W, H)
    out = []
    for step in steps:
        if step[0] == "reset":
            h.reset()
            continue
        a = step[1]
        g = a["guides"]
        prev = g["prev_position"] if (motion and a["motion"]) else None
        mean = h.advance(a["camera"], a["frame"], g["normal"], g["position"], g["coverage"], prev_position=prev, **a["params"])
        out.append(dict(mean=mean, length=h.n.copy(), q=h.q.copy(), kept=h.kept, restarted=h.restarted, frames=h.K,
                        variance=h.variance(), branches=dict(h.branches)))
    return out


def size_of(steps):
    return hc.size_of(steps)
