"""Case table of the scene-update suite: a base scene and a sequence of vertex edits, each handed to
Scene.update_triangles (or, in `rounds`, Scene.update_rounds) on ONE handle that lives through the whole sequence.  The
refit keeps the tree's topology and recomputes every box, the grid, both quantised trees and the frames; the cases are
the ways that can go wrong.  A plain module: no GPU, no tests.

A case is `Case(name, make)`; make() returns `Data(L, sp, tr, steps, order)`: the base records and, per step, the
records `(L, sp, tr)` the handle holds AFTER the step (`order` is the BDPT grouping, sio.object_order).  Everything is
rendered at 48 x 48, depth 4, 4 spp, seed 31 from the Cornell camera, as build_cases.py does.  The base scene is
cornell_with_sphere(2000) (12 wall triangles and a 1860-triangle sphere) unless said otherwise:

  identity        the same vertices again: the refit reproduces the builder's bytes
  turn            the sphere's triangles turned 30 degrees about the sphere's centre, three times (its triangles are
                  recoloured in bands so that a turn shows): every normal changes, so the frames must be recomputed
  out             the sphere moved towards the camera, out of the room by three scene extents: outside the old grid, and
                  it must be visible (the room without the wall behind the Cornell camera, seen from its far end: out_case)
  shrink          the whole scene scaled by 0.25 about the look-at point: the grid tightens
  scramble        the sphere's triangles exchange positions by a seeded permutation (twice): neighbours in the tree are
                  far apart in space.  Base: cornell_random_triangles(3000), the deep irregular tree, with its first 1500
                  small triangles blown up fourfold so that they show
  die-and-return  20 triangles (6 walls, 14 of the sphere) get a NaN coordinate; the next step puts them back elsewhere;
                  a later step makes every triangle dead; the last brings the base scene back
  coincide        the red wall's two triangles made exact copies of the green wall's: two pairs of coincident triangles
                  of different colour, the lowest ordinal must win
  there-and-back  A -> B -> A (B: the sphere lowered and the walls pulled apart)
  tiny-1, -2, -3  scenes of 1, 2 and 3 triangles, each updated twice
  rounds          two spheres added to the base scene; the light moved and dimmed and a sphere moved (update_rounds),
                  then the triangles turned as well (update_triangles): both kinds of update on one handle

  parallel        three triangles under a PARALLEL light, updated once.  PPM_STEP names this step: the photon-mapping
                  render the GPU suite checks.  The bounds handed to photon mapping reach the image through a parallel
                  light's emission plane alone, and hpt_render_ppm with null bounds takes the scene's own, which an
                  update must recompute: the oracle's image under the base scene's bounds differs from the one under the
                  new bounds."""
import collections
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from path_tracing_amd import scene_io as sio                       # noqa: E402
from path_tracing_amd.layouts import SPHERE                        # noqa: E402

Case = collections.namedtuple("Case", "name make")
Data = collections.namedtuple("Data", "L sp tr steps order eye look", defaults=(sio.CORNELL_EYE, sio.CORNELL_LOOK))

W, H, DEPTH, SPP, SEED = 48, 48, 4, 4, 31
NWALL = 12
SPHERE_C = np.array((-0.15, 0.2, 0.45), np.float64)                 # cornell_with_sphere's tessellated sphere
NAN = float("nan")
F32 = np.float32


def camera(name=None, w=W, h=H):
    """The camera record of a case's PT, PPM and guide renders: the Cornell camera, but for `out`."""
    eye, look = (data(name).eye, data(name).look) if name else (sio.CORNELL_EYE, sio.CORNELL_LOOK)
    return sio.make_camera(eye, look, sio.CORNELL_UP, 50.0, w, h)


def base():
    L, sp, tr = sio.cornell_with_sphere(2000)
    assert len(tr) == 1872
    return L, sp, tr


def banded(tr):
    """The sphere's triangles recoloured by longitude band (a function of the triangle, not of where it is)."""
    tr = tr.copy()
    k = (np.arange(len(tr) - NWALL) // 5) % 3
    col = np.array([(0.85, 0.2, 0.2), (0.2, 0.8, 0.25), (0.25, 0.3, 0.9)], F32)[k]
    tr["mtl"]["base_color"][NWALL:] = col
    return tr


def verts(tr):
    return np.stack([tr["v0"], tr["v1"], tr["v2"]], axis=1).astype(np.float64)          # [n, 3, 3]


def with_verts(tr, v, which=slice(None)):
    out = tr.copy()
    v = np.asarray(v).astype(F32)
    for k, name in enumerate(("v0", "v1", "v2")):
        a = out[name].copy()
        a[which] = v[:, k]
        out[name] = a
    return out


def rotate_y(v, centre, degrees):
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return (v - centre) @ R.T + centre


def rotate_z(v, centre, degrees):
    a = np.radians(degrees)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return (v - centre) @ R.T + centre


def _order(sp, tr):
    """The grouping the BDPT steps set BEFORE the updates: the spheres and the first NWALL triangles (the walls) in group 0,
    every other triangle in group 1 -- not the default single group, so an update that dropped the grouping would show."""
    kind, index, group = sio.object_order(None, sp, tr)
    group = group.copy()
    group[len(sp) + NWALL:] = 1
    return kind, index, group


def _data(L, sp, tr, trs):
    return Data(L, sp, tr, [(L, sp, t) for t in trs], _order(sp, tr))


def identity_case():
    L, sp, tr = base()
    return _data(L, sp, tr, [tr.copy()])


def turn_case():
    L, sp, tr = base()
    tr = banded(tr)
    ball = slice(NWALL, None)
    # about an axis tilted out of the tessellation's own, so that the bands sweep across the image
    steps, cur = [], tr
    for k in range(3):
        v = rotate_z(rotate_y(verts(cur)[ball], SPHERE_C, 30.0), SPHERE_C, 30.0)
        cur = with_verts(cur, v, ball)
        steps.append(cur)
    return _data(L, sp, tr, steps)


def scene_extent(tr):
    v = verts(tr).reshape(-1, 3)
    return float((v.max(axis=0) - v.min(axis=0)).max())


OUT_EYE, OUT_LOOK = (0.0, 0.0, 0.95), (0.0, 0.0, -1.0)


def out_case():
    """The room is closed behind the Cornell camera (a wall at z = -1.1, the eye at z = -1), so nothing outside it can be
    seen or lit from there: this case leaves that wall out (1870 triangles) and looks out of the room's open side from
    its far end, where the light falls on what the camera sees.  The sphere goes three scene extents out of the opening,
    six times as large so that it fills a part of it."""
    L, sp, tr = base()
    z = verts(tr)[:NWALL, :, 2]
    behind = np.flatnonzero((z == z.min()).all(axis=1))
    assert len(behind) == 2
    tr = np.delete(tr, behind)
    tr["id"] = np.arange(len(tr))
    nw = NWALL - 2
    ball = slice(nw, None)
    v = verts(tr)[ball]
    ext = scene_extent(tr)
    room_front = float(verts(tr)[:nw].reshape(-1, 3)[:, 2].min())
    c2 = np.array((0.0, 0.0, room_front - 3.0 * ext))
    v = (v - SPHERE_C) * 6.0 + c2
    assert v[..., 2].max() < room_front - 2.0 * ext
    return Data(L, sp, tr, [(L, sp, with_verts(tr, v, ball))], _order(sp, tr), OUT_EYE, OUT_LOOK)


def shrink_case():
    L, sp, tr = base()
    look = np.array(sio.CORNELL_LOOK, np.float64)
    v = (verts(tr) - look) * 0.25 + look
    return _data(L, sp, tr, [with_verts(tr, v)])


def scramble_case():
    L, sp, tr = sio.cornell_random_triangles(3000)
    n_big = 1500
    big = slice(NWALL, NWALL + n_big)
    v = verts(tr)[big]
    cen = v.mean(axis=1, keepdims=True)
    tr = with_verts(tr, (v - cen) * 4.0 + cen, big)
    rng = np.random.default_rng(7)
    steps, cur = [], tr
    for _ in range(2):
        perm = rng.permutation(len(tr) - NWALL)
        cur = with_verts(cur, verts(cur)[NWALL:][perm], slice(NWALL, None))
        steps.append(cur)
    return _data(L, sp, tr, steps)


DIE = list(range(2, 8)) + list(range(400, 414))                  # 6 walls, 14 of the sphere


def die_case():
    L, sp, tr = base()
    a = tr.copy()
    for k, name in enumerate(("v0", "v1", "v2")):
        col = a[name].copy()
        sel = [i for j, i in enumerate(DIE) if j % 3 == k]
        col[sel, k] = NAN
        a[name] = col
    v = verts(tr)[DIE]
    b = with_verts(tr, v * 0.6 + np.array((0.1, -0.1, 0.15)), DIE)
    c = with_verts(tr, np.full((len(tr), 3, 3), NAN))
    return _data(L, sp, tr, [a, b, c, tr.copy()])


def wall_pairs(tr):
    """Indices of two pairs of wall triangles with different base colours: (red-ish pair, green-ish pair)."""
    col = tr["mtl"]["base_color"][:NWALL]
    red = [i for i in range(NWALL) if col[i][0] > 0.5 and col[i][1] < 0.3]
    green = [i for i in range(NWALL) if col[i][1] > 0.5 and col[i][0] < 0.3]
    assert len(red) == 2 and len(green) == 2, (red, green)
    return red, green


def coincide_case():
    L, sp, tr = base()
    red, green = wall_pairs(tr)
    v = verts(tr)
    return _data(L, sp, tr, [with_verts(tr, v[green], red)])


def there_and_back_case():
    L, sp, tr = base()
    v = verts(tr)
    v[NWALL:] += np.array((0.1, -0.35, -0.1))
    v[:NWALL, :, 0] *= 1.6
    b = with_verts(tr, v)
    return _data(L, sp, tr, [b, tr.copy()])


TINY_ROWS = [(-0.4, -0.4, 0.6, 0.4, -0.4, 0.6, 0.0, 0.4, 0.6),
             (-0.45, -0.2, 0.8, 0.0, -0.45, 0.8, -0.3, 0.3, 0.8),
             (0.1, -0.1, 0.4, 0.45, -0.3, 0.5, 0.3, 0.35, 0.45)]
TINY_MATS = [(0.8, 0.3, 0.2, 1.0, 0.0, 0.0), (0.2, 0.7, 0.3, 1.0, 0.0, 0.0), (0.3, 0.3, 0.9, 1.0, 0.0, 0.0)]


def tiny_case(n):
    L, sp, _ = base()
    tr = sio._tris_from(TINY_ROWS[:n], TINY_MATS[:n])
    v = verts(tr)
    a = with_verts(tr, rotate_z(v, np.zeros(3), 60.0) * 0.7 + np.array((0.15, 0.1, -0.2)))
    b = with_verts(tr, rotate_y(v, np.array((0, 0, 0.6)), 35.0) + np.array((-0.2, 0.05, 0.3)))
    return _data(L, sp, tr, [a, b])


def parallel_case():
    """The photon-mapping step's scene: three triangles under a parallel light, whose photons start from a plane placed by
    the scene's bounds -- the one place where hpt_render_ppm's null bounds (the scene's own, recomputed after an update)
    reach the image."""
    tr = sio._tris_from(TINY_ROWS, TINY_MATS)
    L = sio._one_light((0.0, 0.3, -0.5), (0.1, -0.3, 1.0), (1.0, 1.0, 1.0), 180.0, 1, 0.05)
    v = verts(tr)
    a = with_verts(tr, rotate_z(v, np.zeros(3), 60.0) * 0.7 + np.array((0.15, 0.1, -0.2)))
    return _data(L, np.zeros(0, SPHERE), tr, [a])


def rounds_case():
    L, _, tr = base()
    tr = banded(tr)
    sp = np.zeros(2, SPHERE)
    for k, (c, r, col) in enumerate([((0.25, -0.35, 0.3), 0.14, (0.2, 0.6, 0.9)), ((-0.3, -0.38, 0.1), 0.11, (0.9, 0.8, 0.2))]):
        sp[k]["center"] = c; sp[k]["r"] = r
        sp[k]["mtl"]["base_color"] = col; sp[k]["mtl"]["roughness"] = 1.0; sp[k]["id"] = k
    L2, sp2 = L.copy(), sp.copy()
    pos = np.array((0.25, 0.3, 0.2), F32)
    L2[0]["pos"] = pos; L2[0]["light_ball"]["center"] = pos
    L2[0]["illum"] = (0.45, 0.4, 0.3)
    sp2[0]["center"] = (-0.05, 0.1, 0.1)
    sp2[1]["r"] = 0.2
    ball = slice(NWALL, None)
    tr2 = with_verts(tr, rotate_z(rotate_y(verts(tr)[ball], SPHERE_C, 40.0), SPHERE_C, 25.0) + np.array((0.2, -0.3, 0.0)), ball)
    return Data(L, sp, tr, [(L2, sp2, tr), (L2, sp2, tr2)], _order(sp, tr))


def _bind(fn, *a):
    return lambda: fn(*a)


CASES = [
    Case("identity", identity_case),
    Case("turn", turn_case),
    Case("out", out_case),
    Case("shrink", shrink_case),
    Case("scramble", scramble_case),
    Case("die-and-return", die_case),
    Case("coincide", coincide_case),
    Case("there-and-back", there_and_back_case),
    Case("tiny-1", _bind(tiny_case, 1)),
    Case("tiny-2", _bind(tiny_case, 2)),
    Case("tiny-3", _bind(tiny_case, 3)),
    Case("rounds", rounds_case),
    Case("parallel", parallel_case),
]
NAMES = [c.name for c in CASES]
CASE_BY_NAME = {c.name: c for c in CASES}
PPM_STEP = ("parallel", 0)
PPM = dict(eye_depth=4, light_depth=4, spp=1, spl=4096, radius=0.05, seed=5)
SAME_AS_BEFORE = [("identity", 0)]                                   # steps that must NOT change the image
ALL_DEAD = ("die-and-return", 2)
N_DEAD = {("die-and-return", 0): 20, ("die-and-return", 1): 0, ("die-and-return", 2): 1872, ("die-and-return", 3): 0}

_DATA, _SCANS, _TREES = {}, {}, {}


def data(name):
    if name not in _DATA:
        _DATA[name] = CASE_BY_NAME[name].make()
    return _DATA[name]


def records(name, step):
    """(L, sp, tr) the handle holds after `step`; step -1 is the base scene."""
    d = data(name)
    return (d.L, d.sp, d.tr) if step < 0 else d.steps[step]


def is_rounds_step(name, step):
    """The step changes lights or spheres (update_rounds), not triangles."""
    (L0, s0, _), (L1, s1, _) = records(name, step - 1), records(name, step)
    return L0.tobytes() != L1.tobytes() or s0.tobytes() != s1.tobytes()


def is_triangle_step(name, step):
    return records(name, step - 1)[2].tobytes() != records(name, step)[2].tobytes() or not is_rounds_step(name, step)


def scan(oracle_mod, name, step):
    """(image, stats) of the oracle's scan on the records after `step`, once per process, read-only."""
    key = (name, step)
    if key not in _SCANS:
        L, sp, tr = records(name, step)
        img, st = oracle_mod.pt_render(L, sp, tr, camera(name), W, H, DEPTH, SPP, seed=SEED)
        img.setflags(write=False)
        _SCANS[key] = (img, st)
    return _SCANS[key]


def tree(hpt, name, step):
    """The definition's tree after `step` (refit_bvh_host from the base records; step -1: the builder's), once per process."""
    key = (name, step)
    if key not in _TREES:
        d = data(name)
        L, sp, tr = records(name, step)
        _TREES[key] = hpt.export_bvh_host(d.L, d.sp, d.tr) if step < 0 else hpt.refit_bvh_host(d.L, d.sp, d.tr, tr)
    return _TREES[key]


def dead(tr):
    with np.errstate(invalid="ignore", over="ignore"):
        e1 = tr["v1"].astype(F32) - tr["v0"].astype(F32)
        e2 = tr["v2"].astype(F32) - tr["v0"].astype(F32)
    return ~(np.isfinite(e1).all(axis=1) & np.isfinite(e2).all(axis=1))


def changed_share(a, b):
    return float((np.asarray(a) != np.asarray(b)).any(axis=-1).mean())


def all_steps():
    return [(c.name, i) for c in CASES for i in range(len(data(c.name).steps))]
