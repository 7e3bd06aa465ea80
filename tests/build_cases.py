"""Case table of the tree builder's coverage suite: scenes at which csrc/scene_build.cpp can go wrong and the other
tables do not look -- triangle records with NaN, infinite and overflowing coordinates, and finite outliers that stretch
the 16-bit grid.  A plain module: no GPU, no tests.

Every case is `Case(name, make, dark)`; make() returns
    (L, sp, tr, cam_record, W, H, eye_depth, spp, params_kw)
as in pt_cases.py.  The base scene is cornell_with_sphere(2000) (1872 triangles) at 40 x 32, depth 4, 3 spp, seed 31; the
junk triangles are copies of one triangle inside the box with coordinates replaced, appended unless the name says
otherwise.

What the reference's scan does with such a record (oracle/ref_math.hpp, intersect_triangle; the device's hit_triangle is
the same expression): with an edge v1 - v0 or v2 - v0 that has a NaN or infinite component the determinant `a` is
infinite or NaN, so f = 1 / a is 0 or NaN and t = f * (...) is 0 or NaN: no ray hits that triangle.  The builder
(scene_build.cpp, "dead" triangles) keeps such records in the leaves -- the leaf slots stay a permutation of the input --
but out of every box, of the grid and of pad_abs.  A triangle with finite edges is an ordinary one however far it reaches.

Observed on the CPU oracle (lit = share of pixels with a non-zero channel, closest and shadow = rays of the scan) and on its
walk of export_bvh_host's tree (boxes = boxes_closest / 2 / closest_rays: node visits per closest-hit ray; tris =
tris_closest / closest_rays; the gate of SURVEY 8(d) is 3 log2(N) = 32.6 boxes at N = 1872, 10.8 at N = 12).  `before` is
the builder that let every record into the boxes, the grid and pad_abs:
  case            N     lit     closest  shadow   nodes  depth   boxes    tris    before: nodes   boxes    tris
  plain           1872  94.9 %   14263    4678     993    14       6.9     2.3             993     6.9     2.3
  nan-one         1873  94.9 %   14263    4678     994    14       7.0     2.3             996     8.1     2.2
  nan-20-middle   1892  94.9 %   14263    4678    1005    14       7.0     2.3            1006  1006.0  1892.0
  nan-20-front    1892  94.9 %   14263    4678    1005    14       7.0     2.3            1006  1006.0  1892.0
  inf-one         1873  94.9 %   14263    4678     994    14       7.0     2.3            1019  1019.0  1873.0
  inf-30          1902  94.9 %   14263    4678    1009    14       7.0     2.3            1039  1039.0  1902.0
  overflow-span   1875  94.9 %   14263    4678     995    14       7.0     2.3             996   996.0  1875.0
  reach-1e30      1875  74.9 %   11428    3459    1025    13    1025.0  1875.0            1025  1025.0  1875.0
  reach-1e6       1875  92.0 %   13898    4660     996    17     996.0  1875.0             996   996.0  1875.0
  live-overflow   1873  93.8 %   14018    4531     997    13     997.0  1873.0             (the same code path)
  all-nan           12   1.3 %    3840       0       7     3       1.0     0.0               7     1.1     0.2  (dark)
  junk-spheres    1872  95.0 %   14084    4621     993    14       6.9     2.2             993     6.9     2.2
In every row the walk gives the scan's bytes and ray counts, before and after, also with every reciprocal moved 1 or 2 float
neighbours in each of the 8 direction combinations (tests/test_build_cases_cpu.py prints the figures with -s).  The dead
triangles change nothing the scan returns: nan-* , inf-* and overflow-span render plain's image.

reach-1e30, reach-1e6 and live-overflow are the finite outliers: ordinary triangles (finite edges: the scan hits them, the
images differ from plain's) with a vertex far away.  The tree has one 16-bit grid over the scene's extent (DESIGN.md
section 4), so a cell is 1.5e25 resp. 15 wide, every box of the Cornell scene is the same few cells and a ray tests every
node.  Their images are right; their work is not gated.

Dropped: the base scene with every coordinate scaled by 2^-130 (denormal), camera moved likewise.  The oracle's scan
renders nothing there -- the determinant of every triangle underflows to 0 and intersect_triangle's |a| < 1e-6 test
rejects it -- so the case could not tell a right tree from a wrong one.
"""
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

Case = collections.namedtuple("Case", "name make dark")

W, H, DEPTH, SPP, SEED = 40, 32, 4, 3, 31
MAX_TRIS = 2100
NAN, INF = float("nan"), float("inf")
JUNK = (-0.2, -0.3, 0.4, -0.2, -0.25, 0.45, 0.3, -0.3, 0.5)          # v0 v1 v2 of the triangle the junk is made from
JUNK_MAT = (0.8, 0.3, 0.2, 0.5, 0.0, 0.0)


def _base():
    return sio.cornell_with_sphere(2000)


def _cam():
    return sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)


def _case(L, sp, tr):
    tr = tr.copy()
    tr["id"] = np.arange(len(tr))
    assert len(tr) <= MAX_TRIS
    return L, sp, tr, _cam(), W, H, DEPTH, SPP, dict(seed=SEED)


def junk(rows):
    """Triangle records of 9-tuples."""
    return sio._tris_from(rows, [JUNK_MAT] * len(rows))


def _with(coords):
    """JUNK with {position 0..8: value} replaced."""
    r = list(JUNK)
    for k, v in coords.items():
        r[k] = v
    return tuple(r)


def _added(rows, at="end"):
    L, sp, tr = _base()
    k = {"end": len(tr), "middle": len(tr) // 2, "front": 0}[at]
    return _case(L, sp, np.concatenate([tr[:k], junk(rows), tr[k:]]))


def plain_case():
    return _case(*_base())


def nan_one_case():
    return _added([_with({4: NAN})])                                  # v1.y


def nan_20_case(at):
    return _added([(NAN,) * 9] * 20, at)


def inf_one_case():
    return _added([_with({6: INF})])                                  # v2.x


def inf_30_case():
    """-inf in x and +inf in y, in each of the three vertices in turn."""
    return _added([_with({3 * (k % 3): -INF, 3 * (k % 3) + 1: INF}) for k in range(30)])


def overflow_span_case():
    """Finite coordinates whose difference is not: v0.x = -3e38, v1.x = +3e38 (e1.x = +inf in float), and the two other
    ways round."""
    return _added([_with({0: -3e38, 3: 3e38}), _with({0: 3e38, 6: -3e38}), _with({0: -3e38, 3: 3e38, 6: 3e38})])


def reach_case(far):
    """Three ordinary triangles with one vertex at `far` along x, y and z: finite edges, so the scan can hit them."""
    return _added([_with({6: far}), _with({4: far}), _with({8: far})])


def live_overflow_case():
    """One triangle with v0.x = 0, v1.x = -3e38, v2.x = +3e38: both edges are finite, so the
    scan can hit it, but the x extent of its box is not.  pad_abs is then infinite, so is every box, and the grid is
    origin -inf, scale +inf: every plane the walk computes is NaN, fminf / fmaxf drop it, and the walk is a scan of every
    node -- the one way left to hand the device non-finite planes."""
    return _added([_with({0: 0.0, 3: -3e38, 6: 3e38})])


def all_nan_case():
    """12 triangles, each with one NaN coordinate (every position of the record in turn, the first three twice), and the
    base scene's light: nothing to hit."""
    L, sp, _ = _base()
    return _case(L, sp, junk([_with({k % 9: NAN}) for k in range(12)]))


def junk_spheres_case():
    """Spheres are scanned, not in the tree: one with a NaN centre and one with an infinite radius between two ordinary
    ones must leave the tree the base scene's."""
    L, _, tr = _base()
    sp = np.zeros(4, SPHERE)
    for k, (c, r) in enumerate([((0.25, -0.35, 0.3), 0.12), ((NAN, 0.0, 0.3), 0.1), ((0.0, 0.0, 0.5), INF), ((0.3, 0.2, 0.7), 0.08)]):
        sp[k]["center"] = c; sp[k]["r"] = r
        sp[k]["mtl"]["base_color"] = (0.2, 0.6, 0.9); sp[k]["mtl"]["roughness"] = 1.0; sp[k]["id"] = k
    return _case(L, sp, tr)


def denormal_case():
    """NOT in the table (module docstring): every coordinate times 2^-130, the camera's eye and image plane moved along."""
    s = np.float32(2.0 ** -130)
    L, sp, tr = _base()
    tr = tr.copy(); L = L.copy()
    for k in ("v0", "v1", "v2"):
        tr[k] = tr[k] * s
    L["pos"] *= s; L["light_ball"]["center"] *= s; L["light_ball"]["r"] *= s
    cam = _cam().copy()
    eye = np.asarray(cam["eye"], np.float32).copy()
    cam["UL"] = (np.asarray(cam["UL"], np.float32) - eye) + eye * s
    cam["eye"] = eye * s
    return L, sp, tr, cam, W, H, DEPTH, SPP, dict(seed=SEED)


def _bind(fn, *a):
    return lambda: fn(*a)


CASES = [
    Case("plain", plain_case, None),
    Case("nan-one", nan_one_case, None),
    Case("nan-20-middle", _bind(nan_20_case, "middle"), None),
    Case("nan-20-front", _bind(nan_20_case, "front"), None),
    Case("inf-one", inf_one_case, None),
    Case("inf-30", inf_30_case, None),
    Case("overflow-span", overflow_span_case, None),
    Case("reach-1e30", _bind(reach_case, 1e30), None),
    Case("reach-1e6", _bind(reach_case, 1e6), None),
    Case("live-overflow", live_overflow_case, None),
    Case("all-nan", all_nan_case, "no triangle can be hit: only the rays that meet the light ball return anything"),
    Case("junk-spheres", junk_spheres_case, None),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
DARK = ["all-nan"]
FINITE_OUTLIERS = ["reach-1e30", "reach-1e6", "live-overflow"]       # correctness only: one 16-bit grid over the scene's extent
NON_FINITE_GRID = ["live-overflow"]
SAME_TREE_AS_PLAIN = ["junk-spheres"]

_REFERENCE = {}
_TREES = {}


def dead(tr):
    """Which triangles no ray can hit: an edge v1 - v0 or v2 - v0 with a component that is not finite in float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        e1 = tr["v1"].astype(np.float32) - tr["v0"].astype(np.float32)
        e2 = tr["v2"].astype(np.float32) - tr["v0"].astype(np.float32)
    return ~(np.isfinite(e1).all(axis=1) & np.isfinite(e2).all(axis=1))


def oracle_render(oracle_mod, args, **extra):
    L, sp, tr, cam, w, h, depth, spp, kw = args
    return oracle_mod.pt_render(L, sp, tr, cam, w, h, depth, spp, **dict(kw, **extra))


def reference(oracle_mod, name):
    """(args, image, stats) of a case by the oracle's scan, computed once per process and shared; callers must not write
    to them."""
    if name not in _REFERENCE:
        args = CASE_BY_NAME[name].make()
        img, st = oracle_render(oracle_mod, args)
        img.setflags(write=False)
        _REFERENCE[name] = (args, img, st)
    return _REFERENCE[name]


def tree(hpt, name):
    """The tree the library builds for a case's scene (export_bvh_host: no device needed), once per process."""
    if name not in _TREES:
        _TREES[name] = hpt.export_bvh_host(*CASE_BY_NAME[name].make()[:3])
    return _TREES[name]


def lit_share(img):
    return float((np.asarray(img) != 0).any(axis=-1).mean())
