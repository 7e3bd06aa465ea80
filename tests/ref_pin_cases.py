"""Inputs of the reference pin (tests/golden/make_ref_golden.py): the edge records of the function table, the tiny scenes
with their rays and segments, and the render cases.  A plain module: no GPU, no tests, and it never touches the
reference -- the generator hands what is built here to the reference's own code and stores inputs and answers together in
tests/golden/ref_*.npz, so the tests read fixtures only.

Every scene holds at most 64 primitives (spheres + light balls + triangles), at most 4096 rays and 4096 segments.
  input, mis_test   the reference's two scene files
  ties              two coincident triangles of different material, a quad hit exactly on its shared diagonal and on its
                    outer edges and corners, by axis-parallel rays with two zero components (the scan's first-of-equals rule)
  slivers           zero-area triangles (collinear, two equal vertices, a point), needle slivers, a sliver seen edge-on
  spheres           a sphere seen from its inside (origins in it, diffuse and glass), rays tangent to a sphere to the last
                    bit, concentric spheres, a sphere cut by a triangle
  epsilon           origins lying on a surface and 1e-4 -+ a few float neighbours off it, along the normal and grazing;
                    segments whose blocker sits at the 1e-3 near bound and at dist - 1e-3, -+ a few float neighbours
  axis              the Cornell box with its two small boxes: axis-parallel rays and rays with one or two exact zeros,
                    from origins on a lattice that includes wall planes, edges and corners
  shell             a light ball shut in an opaque sphere and another one shut in an opaque box of triangles, beside a free
                    cone light: nothing outside sees the shut-in balls, every shadow segment towards them is blocked
  sky               an open floor with boxes and spheres of rough glass, eta 2.4 glass, a mirror and a conductor under one
                    parallel light, one narrow cone light and one 360-degree ball
"""
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from path_tracing_amd import scene_io as sio                                 # noqa: E402
from path_tracing_amd.layouts import SPHERE                                  # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(_HERE, "golden")
MAX_PRIMS, MAX_RAYS = 64, 4096
U_TOP = f32(1.0) - f32(2.0 ** -24)                 # the largest uniform below 1

DIFFUSE = (0.7, 0.6, 0.5, 1.0, 0.0, 0.0)
ROUGH = (0.2, 0.5, 0.8, 0.3, 0.0, 0.0)
CONDUCTOR = (0.9, 0.7, 0.3, 0.2, 0.9, 0.0)
MIRROR = (1.0, 1.0, 1.0, 0.0, 1.0, 0.0)
GLASS = (1.0, 1.0, 1.0, 0.0, 0.0, 1.5)
DIAMOND = (0.9, 0.95, 1.0, 0.0, 0.0, 2.4)
ROUGH_GLASS = (1.0, 1.0, 1.0, 0.4, 0.0, 1.5)


# ---- function records -----------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)


def _reflect32(wo, N):
    """-wo reflected about N in float32, in the operand order of reflect(I, N) = I - N * 2 * dot(N, I) with I = -wo."""
    I = (-wo).astype(f32)
    d = ((N[:, 0] * I[:, 0]).astype(f32) + (N[:, 1] * I[:, 1]).astype(f32)).astype(f32)
    d = (d + (N[:, 2] * I[:, 2]).astype(f32)).astype(f32)
    return (I - ((N * f32(2.0)).astype(f32) * d[:, None]).astype(f32)).astype(f32)


def _neighbours(x, ks):
    out = []
    for k in ks:
        v = f32(x)
        for _ in range(abs(k)):
            v = np.nextafter(v, f32(np.inf) if k > 0 else f32(-np.inf), dtype=f32)
        out.append(v)
    return np.array(out, f32)


def tir_cos(eta):
    """cos of the critical angle inside a medium of index eta against air, in float32 the way FrDielectric gets there."""
    return f32(np.sqrt(f32(1.0) - f32(1.0) / (f32(eta) * f32(eta))))


N_EDGE = 640
_MATS = [DIFFUSE, ROUGH, CONDUCTOR, MIRROR, GLASS, DIAMOND, ROUGH_GLASS, (0.95, 0.93, 0.88, 0.3, 0.8, 0.0)]


def edge_records():
    """640 records at the edges the seeded ones of kat_records.records do not reach; layout of kat_records.  Eight
    blocks of 80: roughness 0 / 5e-4 / 1; eta exactly 1; wo at 89.99 degrees to N; wo at 90 degrees; wo below N;
    wi = reflect(wo) exactly; cosThetaI at -+1 and at the total-internal-reflection threshold of 1.5 and 2.4 -+ float
    neighbours (as the Fresnel argument and as wo of a smooth dielectric); uniforms 0 and 1 - 2^-24 in every combination."""
    rng = np.random.default_rng(20240)
    n = 80
    blocks, names = [], []

    def base(name):
        r = np.zeros((n, 24), f32)
        r[:, 0:6] = np.array([_MATS[k % len(_MATS)] for k in range(n)], f32)
        N = _unit(rng.normal(size=(n, 3)))
        N[0::8] = (0, 0, 1); N[1::8] = (0, 0, -1); N[2::8] = (0, 1, 0); N[3::8] = (1, 0, 0)
        wo = _unit(rng.normal(size=(n, 3)))
        flip = np.einsum("ij,ij->i", wo.astype(np.float64), N.astype(np.float64)) < 0
        wo[flip] *= -1
        wi = _unit(rng.normal(size=(n, 3)))
        r[:, 6:9], r[:, 9:12], r[:, 12:15] = N, wo, wi
        r[:, 15:18] = (rng.integers(0, 1 << 24, (n, 3)) / f32(1 << 24)).astype(f32)
        r[:, 18] = rng.choice([1.0, 1.5, 2.4], n)
        r[:, 19] = rng.uniform(-1.0, 1.0, n)
        r[:, 20] = rng.choice([1.0, 1.5, 2.4], n)
        r[:, 21] = rng.choice([1.0, 1.5, 2.4], n)
        names.extend([name] * n)
        return r

    def tangent_of(N):
        a = np.where(np.abs(N[:, 2:3]) < 0.9, np.array([[0, 0, 1.0]]), np.array([[1.0, 0, 0]]))
        return _unit(np.cross(N.astype(np.float64), a))

    r = base("roughness")
    r[:, 3] = np.array([0.0, 5e-4, 1.0, 1e-3, f32(1e-3) - f32(1e-10), 0.01], f32)[np.arange(n) % 6]
    r[:, 4] = np.array([0.0, 0.5, 1.0, 0.99, 0.995, 0.01, 0.005], f32)[np.arange(n) % 7]
    r[:, 5] = np.array([0.0, 1.5, 0.0, 2.4, 0.0], f32)[np.arange(n) % 5]
    r[70:75, 0] = -0.5; r[75:80, 1] = np.inf                     # colours the guards must refuse
    blocks.append(r)

    r = base("eta-one")
    r[:, 5] = 1.0
    r[:, 3] = np.array([0.0, 0.0, 0.4, 5e-4], f32)[np.arange(n) % 4]
    r[:, 4] = 0.0
    r[:, 18] = np.array([1.0, 1.0, 1.5], f32)[np.arange(n) % 3]
    r[:, 20] = 1.0; r[:, 21] = 1.0
    blocks.append(r)

    for name, deg in (("wo-89.99", 89.99), ("wo-90", 90.0)):
        r = base(name)
        N = r[:, 6:9]
        t = tangent_of(N).astype(np.float64)
        a = math.radians(deg)
        wo = (math.cos(a) * N.astype(np.float64) + math.sin(a) * t) if deg != 90.0 else t
        r[:, 9:12] = _unit(wo)
        if deg == 90.0:             # exact zeros for the axis normals: wo.N == 0 to the bit
            r[0::8, 9:12] = (1, 0, 0); r[1::8, 9:12] = (0, 1, 0); r[2::8, 9:12] = (0, 0, 1); r[3::8, 9:12] = (0, 1, 0)
            r[n // 2:, 12:15] = tangent_of(N)[n // 2:]           # wi in the plane as well
        blocks.append(r)

    r = base("wo-below")
    r[:, 9:12] *= -1
    r[:, 18] = np.array([1.0, 1.5, 2.4], f32)[np.arange(n) % 3]
    blocks.append(r)

    r = base("wi-reflect")
    r[:, 12:15] = _reflect32(r[:, 9:12], r[:, 6:9])
    r[n // 2:, 9:12] *= -1                                       # half of them from below
    r[n // 2:, 12:15] = _reflect32(r[n // 2:, 9:12], r[n // 2:, 6:9])
    blocks.append(r)

    r = base("fresnel-edges")
    ks = [-2, -1, 0, 1, 2]
    cosv = np.concatenate([[1.0, -1.0, 0.0, -0.0, 1.2, -1.2], _neighbours(1.0, [-1]), _neighbours(-1.0, [1]),
                           _neighbours(tir_cos(1.5), ks), _neighbours(tir_cos(2.4), ks),
                           -_neighbours(tir_cos(1.5), ks), -_neighbours(tir_cos(2.4), ks)]).astype(f32)      # 28 values
    etas = [(1.0, 1.5), (1.5, 1.0), (1.0, 2.4), (2.4, 1.0)]
    for k in range(n):
        r[k, 19] = cosv[k % len(cosv)]
        r[k, 20], r[k, 21] = etas[(k // len(cosv) + k) % 4]
    # the same thresholds through bsdf_sample: smooth glass, N = +z, wo = (s, 0, -c) leaving the medium it is inside of
    for k in range(40, n):
        eta = 1.5 if k % 2 == 0 else 2.4
        c = _neighbours(tir_cos(eta), [ks[(k // 2) % 5]])[0]
        s = f32(np.sqrt(np.float64(1.0) - np.float64(c) * np.float64(c)))
        r[k, 0:6] = GLASS if eta == 1.5 else DIAMOND
        r[k, 6:9] = (0, 0, 1)
        r[k, 9:12] = (s, 0, -c) if k % 4 < 2 else (0, -s, -c)
        r[k, 15] = (0.0, 0.5, U_TOP)[(k // 10) % 3]
        r[k, 18] = eta
    blocks.append(r)

    r = base("uniform-edges")
    for k in range(n):
        r[k, 15] = (0.0, U_TOP)[k & 1]; r[k, 16] = (0.0, U_TOP)[(k >> 1) & 1]; r[k, 17] = (0.0, U_TOP)[(k >> 2) & 1]
    r[:, 0:6] = np.array([_MATS[(k >> 3) % len(_MATS)] for k in range(n)], f32)
    blocks.append(r)

    rec = np.concatenate(blocks).astype(f32)
    assert rec.shape == (N_EDGE, 24) and len(names) == N_EDGE
    return np.array(names), rec


def committed_records():
    """The 640 records tests/golden/kat_functions.npz holds (kat_records.records(64, 7))."""
    g = np.load(os.path.join(GOLDEN, "kat_functions.npz"))
    return np.ascontiguousarray(g["records"], f32)


# ---- scenes ---------------------------------------------------------------------------------------------------------
def _sphere(center, r, mat, k):
    s = np.zeros(1, SPHERE)
    s[0]["center"] = center; s[0]["r"] = r
    s[0]["mtl"]["base_color"] = mat[0:3]; s[0]["mtl"]["roughness"] = mat[3]; s[0]["mtl"]["metallic"] = mat[4]; s[0]["mtl"]["eta"] = mat[5]
    s[0]["mtl"]["type"] = 1 if mat[5] > 0 else (2 if mat[4] > 0 else 3)
    s[0]["id"] = k
    return s


def _spheres(rows):
    return np.concatenate([_sphere(c, r, m, k) for k, (c, r, m) in enumerate(rows)]) if rows else np.zeros(0, SPHERE)


def _walls(mats=None):
    rows = [t for _, tl in sio._CORNELL_WALLS for t in tl]
    m = [m6 for m6, tl in sio._CORNELL_WALLS for _ in tl]
    return rows, (m if mats is None else [mats] * len(rows))


FLOOR = [(-2.0, -0.5, -2.0, -2.0, -0.5, 3.0, 2.0, -0.5, 3.0), (-2.0, -0.5, -2.0, 2.0, -0.5, 3.0, 2.0, -0.5, -2.0)]
QUAD = [(-0.25, -0.25, 0.5, 0.25, -0.25, 0.5, 0.25, 0.25, 0.5), (-0.25, -0.25, 0.5, 0.25, 0.25, 0.5, -0.25, 0.25, 0.5)]


def scene_file(name):
    sc = sio.load_scene(os.path.join(GOLDEN, "scenes", name + ".txt"))
    return sio.flatten_for_pt(sc), sc


def scene_ties():
    twin = (-0.4, -0.1, 0.8, 0.1, -0.1, 0.8, -0.15, 0.4, 0.8)
    rows = FLOOR + QUAD + [twin, twin, twin] + [(0.25, -0.25, 0.5, 0.6, -0.25, 0.5, 0.6, 0.25, 0.5)]
    mats = [DIFFUSE, DIFFUSE, ROUGH, CONDUCTOR, (0.9, 0.1, 0.1, 1.0, 0.0, 0.0), (0.1, 0.9, 0.1, 1.0, 0.0, 0.0), GLASS, DIFFUSE]
    L = np.concatenate([sio._one_light((0.0, 0.45, 0.1), (0.0, -1.0, 0.3), (1.0, 1.0, 1.0), 180.0, 0, 0.05),
                        sio._one_light((0.3, 0.3, -0.2), (0.0, -1.0, 0.0), (0.5, 0.4, 0.3), 360.0, 0, 0.03)])
    return L, np.zeros(0, SPHERE), sio._tris_from(rows, mats)


def scene_slivers():
    rows, mats = _walls()
    rows += [(-0.3, -0.2, 0.3, 0.0, 0.0, 0.4, 0.3, 0.2, 0.5),              # collinear
             (0.1, -0.3, 0.2, 0.1, -0.3, 0.2, 0.3, 0.1, 0.6),              # v0 == v1
             (-0.2, 0.25, 0.5, -0.2, 0.25, 0.5, -0.2, 0.25, 0.5),          # a point
             (-0.4, -0.3, 0.6, 0.4, -0.3, 0.6, 0.4, -0.3 + 1e-5, 0.6),     # a needle 1e-5 high
             (-0.4, 0.0, 0.3, 0.4, 0.0, 0.3, 0.0, 1e-3, 0.3),              # a needle 1e-3 high
             (-0.3, 0.1, 0.2, 0.3, 0.1, 0.9, 0.0, 0.1, 0.55 + 1e-4),       # nearly collinear
             (0.0, -0.4, 0.1, 0.0, 0.4, 0.1, 0.0, 0.0, 0.9),               # edge-on to rays in the plane x = 0
             (1e-7, -0.2, 0.4, 2e-7, 0.2, 0.4, 1.5e-7, 0.0, 0.7)]          # determinant inside the +-1e-6 reject band
    mats += [DIFFUSE, ROUGH, DIFFUSE, CONDUCTOR, DIFFUSE, GLASS, ROUGH, DIFFUSE]
    L = sio._one_light((0.0, 0.4, 0.2), (0.0, -1.0, 0.0), (1.0, 1.0, 1.0), 180.0, 0, 0.08)
    return L, np.zeros(0, SPHERE), sio._tris_from(rows, mats)


def scene_spheres():
    sp = _spheres([((0.0, 0.0, 0.0), 2.0, DIFFUSE), ((0.0, 0.0, 0.5), 0.3, GLASS), ((0.0, 0.0, 0.5), 0.15, DIAMOND),
                   ((0.6, 0.0, 0.5), 0.25, MIRROR), ((-0.6, 0.0, 0.5), 0.25, ROUGH_GLASS), ((0.0, 0.6, 0.5), 0.2, CONDUCTOR),
                   ((0.0, -0.7, 0.5), 0.2, ROUGH)])
    rows = [(-0.9, -0.7, 0.5, -0.3, -0.7, 0.5, -0.6, 0.7, 0.5), (-1.0, -0.9, -1.0, 1.0, -0.9, -1.0, 0.0, -0.9, 1.5)]
    L = np.concatenate([sio._one_light((0.0, 1.2, -0.5), (0.0, -1.0, 0.4), (3.0, 3.0, 3.0), 180.0, 0, 0.1),
                        sio._one_light((0.9, 0.2, -0.8), (-1.0, 0.0, 1.0), (1.0, 0.8, 0.6), 40.0, 0, 0.05)])
    return L, sp, sio._tris_from(rows, [DIFFUSE, ROUGH])


def scene_epsilon():
    rows = FLOOR + [(-0.5, -0.5, 1.0, 0.5, -0.5, 1.0, 0.0, 0.5, 1.0)]
    sp = _spheres([((0.0, 0.0, 0.0), 0.25, DIFFUSE), ((1.0, 0.0, 0.0), 0.25, GLASS)])
    L = sio._one_light((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (2.0, 2.0, 2.0), 180.0, 0, 0.1)
    return L, sp, sio._tris_from(rows, [DIFFUSE, DIFFUSE, ROUGH])


def scene_axis():
    return sio.cornell_diffuse()


def scene_shell():
    rows = FLOOR + sio._box_tris(0.5, 0.6, 0.15, -0.1, 0.2, 0.3)
    mats = [DIFFUSE, DIFFUSE] + [ROUGH] * 12
    sp = _spheres([((-0.5, 0.1, 0.6), 0.2, DIFFUSE), ((0.0, -0.3, 0.3), 0.15, GLASS)])
    L = np.concatenate([sio._one_light((-0.5, 0.1, 0.6), (0.0, -1.0, 0.0), (5.0, 5.0, 5.0), 180.0, 0, 0.05),     # in the sphere
                        sio._one_light((0.5, 0.05, 0.6), (0.0, -1.0, 0.0), (5.0, 5.0, 5.0), 360.0, 0, 0.05),     # in the box
                        sio._one_light((0.0, 0.8, 0.2), (0.1, -1.0, 0.2), (1.0, 1.0, 1.0), 60.0, 0, 0.06)])
    return L, sp, sio._tris_from(rows, mats)


def scene_sky():
    rows = FLOOR + sio._box_tris(-0.3, 0.5, 0.12, -0.5, -0.2, 0.4) + sio._box_tris(0.35, 0.7, 0.1, -0.5, -0.1, 1.1)
    mats = [DIFFUSE, ROUGH] + [ROUGH_GLASS] * 12 + [CONDUCTOR] * 12
    sp = _spheres([((0.0, -0.3, 0.3), 0.2, DIAMOND), ((0.45, -0.35, 0.2), 0.15, MIRROR), ((-0.5, -0.38, 0.1), 0.12, ROUGH_GLASS),
                   ((0.1, -0.42, 0.9), 0.08, GLASS)])
    L = np.concatenate([sio._one_light((0.0, 2.0, 0.0), (0.3, -1.0, 0.2), (0.8, 0.8, 0.7), 0.0, 1, 0.05),        # parallel
                        sio._one_light((-0.4, 0.5, 0.0), (0.3, -1.0, 0.4), (2.0, 1.5, 1.0), 25.0, 0, 0.04),      # narrow cone
                        sio._one_light((0.5, 0.3, 0.9), (0.0, -1.0, 0.0), (0.5, 0.7, 1.0), 360.0, 0, 0.03)])
    return L, sp, sio._tris_from(rows, mats)


# ---- rays and segments ----------------------------------------------------------------------------------------------
def _bbox(L, sp, tr):
    pts = [tr[k].reshape(-1, 3) for k in ("v0", "v1", "v2")] if len(tr) else []
    for a in (sp, L["light_ball"] if len(L) else sp[:0]):
        if len(a):
            pts += [a["center"] - a["r"][:, None], a["center"] + a["r"][:, None]]
    p = np.concatenate(pts).astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    return np.maximum(lo, -1.5), np.minimum(hi, 1.5)


def _norm32(d):
    d = np.asarray(d, f32)
    n2 = ((d[:, 0] * d[:, 0]).astype(f32) + (d[:, 1] * d[:, 1]).astype(f32)).astype(f32)
    n2 = (n2 + (d[:, 2] * d[:, 2]).astype(f32)).astype(f32)
    return (d / np.sqrt(n2).astype(f32)[:, None]).astype(f32)


def generic_rays(L, sp, tr, seed, n_rand=250, n_seg=300):
    """Random rays from random points of the scene's box, rays at the vertices and centres of the primitives, and
    segments between random points and towards the lights."""
    rng = np.random.default_rng(seed)
    lo, hi = _bbox(L, sp, tr)
    o = rng.uniform(lo, hi, (n_rand, 3)).astype(f32)
    d = _unit(rng.normal(size=(n_rand, 3)))
    targets = []
    if len(tr):
        targets += [tr["v0"], tr["v1"], tr["v2"], ((tr["v0"] + tr["v1"]) * f32(0.5)).astype(f32),
                    ((tr["v0"].astype(np.float64) + tr["v1"] + tr["v2"]) / 3.0).astype(f32)]
    if len(sp):
        targets += [sp["center"], (sp["center"] + sp["r"][:, None] * np.array([1, 0, 0], f32)).astype(f32)]
    if len(L):
        targets += [L["pos"]]
    tg = np.concatenate(targets).astype(f32)
    eyes = np.array([[0.0, 0.0, -1.0], [0.3, 0.2, -0.7], [-0.2, 0.4, 0.1]], f32)
    o2 = np.repeat(eyes, len(tg), axis=0)
    d2 = np.tile(tg, (len(eyes), 1)) - o2
    keep = np.abs(d2).sum(1) > 0
    o_all = np.concatenate([o, o2[keep]])
    d_all = np.concatenate([d, _norm32(d2[keep])])
    p1 = rng.uniform(lo, hi, (n_seg, 3)).astype(f32)
    p2 = rng.uniform(lo, hi, (n_seg, 3)).astype(f32)
    if len(L):
        k = n_seg // 2
        lp = L["pos"][rng.integers(0, len(L), k)]
        p2[:k] = (lp + L["light_ball"]["r"][0] * _unit(rng.normal(size=(k, 3)))).astype(f32)
    return o_all, d_all, p1, p2


def _lattice_axis_rays(vals, dirs):
    g = np.array([(x, y, z) for x in vals for y in vals for z in vals], f32)
    o = np.repeat(g, len(dirs), axis=0)
    d = np.tile(np.asarray(dirs, f32), (len(g), 1))
    return o, d


def special_rays(name, L, sp, tr):
    """(origins, dirs, p1, p2) of the scene's own edge: see the module docstring."""
    o, d, p1, p2 = [], [], [], []
    if name == "ties":
        # points on the quad's diagonal, edges and corners, and on the twin triangle, seen head-on from both sides
        pts = [(x, x, 0.5) for x in (-0.25, -0.125, 0.0, 0.0625, 0.25)] + [(0.25, y, 0.5) for y in (-0.25, 0.0, 0.1, 0.25)]
        pts += [(-0.25, 0.1, 0.5), (0.0, -0.25, 0.5), (0.1, 0.25, 0.5), (0.6, 0.0, 0.5)]
        pts += [(-0.4, -0.1, 0.8), (0.1, -0.1, 0.8), (-0.15, 0.4, 0.8), (-0.15, 0.0, 0.8), (-0.15, -0.1, 0.8)]
        for p in pts:
            o += [(p[0], p[1], p[2] - 1.0), (p[0], p[1], p[2] + 1.0), (p[0], p[1], -0.25)]
            d += [(0, 0, 1), (0, 0, -1), (0, 0, 1)]
            p1 += [(p[0], p[1], p[2] - 1.0), (p[0], p[1], p[2] + 0.5)]
            p2 += [(p[0], p[1], p[2] + 1.0), (p[0], p[1], p[2] - 0.5)]
        # along the quad's plane
        o += [(-1.0, 0.0, 0.5), (0.0, -1.0, 0.5), (-1.0, -1.0, 0.5)]
        d += [(1, 0, 0), (0, 1, 0)] + [tuple(_norm32([(1, 1, 0)])[0])]
    elif name == "slivers":
        for x in np.linspace(-0.4, 0.4, 33):
            for y, z in ((-0.3, 0.6), (-0.3 + 5e-6, 0.6), (0.0, 0.3), (5e-4, 0.3), (0.1, 0.55)):
                o.append((x, y, z - 0.7)); d.append((0, 0, 1))
                p1.append((x, y, z - 0.7)); p2.append((x, y, z + 0.3))
        for z in np.linspace(0.1, 0.9, 17):                       # in the plane of the edge-on triangle
            o += [(0.0, -0.45, z), (0.0, 0.0, -0.5)]; d += [(0, 1, 0), tuple(_norm32([(0, 0.1, z + 0.5)])[0])]
        for y in np.linspace(-0.2, 0.2, 9):                       # at the triangle of the reject band
            o.append((-0.4, y, 0.5)); d.append((1, 0, 0))
            p1.append((-0.4, y, 0.5)); p2.append((0.4, y, 0.5))
    elif name == "spheres":
        rng = np.random.default_rng(5)
        for c, r in ((np.array([0.0, 0.0, 0.5]), 0.3), (np.array([0.0, 0.0, 0.5]), 0.15), (np.array([-0.6, 0.0, 0.5]), 0.25)):
            inside = (c + r * 0.9 * rng.uniform(-0.55, 0.55, (60, 3))).astype(f32)          # origins inside the ball
            o += list(map(tuple, inside)); d += list(map(tuple, _unit(rng.normal(size=(60, 3)))))
            p1 += list(map(tuple, inside)); p2 += list(map(tuple, (c + 1.5 * _unit(rng.normal(size=(60, 3)))).astype(f32)))
            o.append(tuple(c.astype(f32))); d.append((0, 0, 1))                                  # from the centre
        # tangent rays: z-parallel lines at x = centre.x + r -+ neighbours, for the balls whose centre and radius are exact
        for cx, r in ((0.6, 0.25), (0.0, 2.0), (0.0, 0.3)):
            for x in _neighbours(f32(cx) + f32(r), [-3, -2, -1, 0, 1, 2, 3]):
                o += [(x, 0.0, -3.0), (x, 0.0, 3.0)]; d += [(0, 0, 1), (0, 0, -1)]
                p1.append((x, 0.0, -1.0)); p2.append((x, 0.0, 1.5))
        for y in _neighbours(f32(-0.7) + f32(0.2), [-2, -1, 0, 1, 2]):
            o.append((-1.5, y, 0.5)); d.append((1, 0, 0))
    elif name == "epsilon":
        # the floor y = -0.5, the wall z = 1, the ball of radius 0.25 at the origin: origins on them and 1e-4 off them
        offs = np.concatenate([[0.0], _neighbours(1e-4, [-2, -1, 0, 1, 2]), _neighbours(1e-3, [-2, -1, 0, 1, 2]), [2e-4, 5e-5]]).astype(f32)
        graze = _norm32([(1, 0, 0), (1, 1e-4, 0), (1, -1e-4, 0), (0.6, 0.0, 0.8)])
        for e in offs:
            for x in (-0.3, 0.1):
                y = f32(-0.5) + e
                for dd in ((0, 1, 0), (0, -1, 0), tuple(graze[0]), tuple(graze[1]), tuple(graze[2])):
                    o.append((x, y, 0.3)); d.append(dd)
                z = f32(1.0) - e
                for dd in ((0, 0, 1), (0, 0, -1), tuple(graze[3])):
                    o.append((x * 0.5, -0.1, z)); d.append(dd)
                o.append((0.0, f32(0.25) + e, 0.0)); d.append((0, -1, 0))
                o.append((0.0, f32(0.25) - e, 0.0)); d.append((0, 1, 0))
        # segments along +z from (x, y, 0) that cross the wall z = 1: the blocker at the near bound, the far bound and between
        for k in range(-4, 5):
            near = _neighbours(1e-3, [k])[0]
            p1.append((0.1, -0.1, f32(1.0) - near)); p2.append((0.1, -0.1, 2.0))
            far = _neighbours(1.0 + 1e-3, [k])[0]
            p1.append((0.1, -0.1, 0.0)); p2.append((0.1, -0.1, far))
            p1.append((0.1, -0.1, f32(1.0) - f32(2e-3) + f32(k) * f32(1e-7))); p2.append((0.1, -0.1, f32(1.0) + f32(1e-3)))
        for x in np.linspace(0.8, 1.2, 9):                               # through the glass ball only, and through both
            p1.append((x, 0.0, -1.0)); p2.append((x, 0.0, 0.9))
        p1 += [(-1.0, 0.0, 0.0), (-1.0, 0.1, 0.0)]; p2 += [(2.0, 0.0, 0.0), (2.0, 0.1, 0.0)]
    elif name == "axis":
        vals = [-0.5, -0.4, -0.25, 0.0, 0.3, 0.5]
        dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
        dirs += list(map(tuple, _norm32([(1, 1, 0), (1, 0, -1), (0, -1, 1), (-1, 2, 0)])))
        oo, dd = _lattice_axis_rays(vals, dirs)
        o += list(map(tuple, oo)); d += list(map(tuple, dd))
        g = np.array([(x, y, z) for x in vals for y in vals for z in vals], f32)
        p1 += list(map(tuple, g)); p2 += list(map(tuple, g[::-1]))
        p1 += list(map(tuple, g[:-1])); p2 += list(map(tuple, g[1:]))
    elif name == "shell":
        rng = np.random.default_rng(9)
        out = np.array([[0.0, 0.5, -0.5], [0.0, -0.45, 0.0], [1.0, 0.3, 0.6], [-1.0, 0.3, 0.6]], f32)
        for c in ((-0.5, 0.1, 0.6), (0.5, 0.05, 0.6)):
            tgt = (np.asarray(c) + 0.05 * _unit(rng.normal(size=(40, 3)))).astype(f32)
            for e in out:
                o += [tuple(e)] * len(tgt); d += list(map(tuple, _norm32(tgt - e)))
                p1 += [tuple(e)] * len(tgt); p2 += list(map(tuple, tgt))
            ins = (np.asarray(c) + 0.09 * _unit(rng.normal(size=(40, 3)))).astype(f32)        # between the ball and its shell
            o += list(map(tuple, ins)); d += list(map(tuple, _unit(rng.normal(size=(40, 3)))))
            p1 += list(map(tuple, ins)); p2 += list(map(tuple, tgt))
    elif name == "sky":
        # the shadow segments of a parallel light: 1e4 long, from points just above the floor and around the objects
        ld = _norm32(-L["dir"][:1])[0]
        for x in np.linspace(-0.9, 0.9, 13):
            for z in np.linspace(-0.4, 1.2, 11):
                a = np.array([x, -0.5 + 1e-4, z], f32)
                p1.append(tuple(a)); p2.append(tuple((a + (ld * f32(1e4)).astype(f32)).astype(f32)))
                o.append(tuple(a)); d.append(tuple(ld))
    o = np.asarray(o, f32).reshape(-1, 3); d = np.asarray(d, f32).reshape(-1, 3)
    p1 = np.asarray(p1, f32).reshape(-1, 3); p2 = np.asarray(p2, f32).reshape(-1, 3)
    return o, d, p1, p2


CAMERAS = {   # eye, look_at, view_up of the render cases (input / mis_test use their files' own)
    "ties": ((0.1, 0.2, -1.0), (0.0, 0.0, 0.6), (0, 1, 0)),
    "slivers": (sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP),
    "spheres": ((0.0, 0.3, -1.2), (0.0, 0.0, 0.5), (0, 1, 0)),
    "epsilon": ((0.5, 0.4, -1.5), (0.3, -0.1, 0.3), (0, 1, 0)),
    "axis": (sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP),
    "shell": ((0.0, 0.4, -1.0), (0.0, 0.0, 0.6), (0, 1, 0)),
    "sky": ((0.0, 0.1, -1.2), (0.0, -0.3, 0.5), (0, 1, 0)),
}
SCENES = ["input", "mis_test", "ties", "slivers", "spheres", "epsilon", "axis", "shell", "sky"]
_BUILDERS = dict(ties=scene_ties, slivers=scene_slivers, spheres=scene_spheres, epsilon=scene_epsilon, axis=scene_axis,
                 shell=scene_shell, sky=scene_sky)


def scene(name):
    """-> (L, sp, tr, (eye, look_at, view_up))"""
    if name in ("input", "mis_test"):
        (L, sp, tr), sc = scene_file(name)
        cam = (sc.eye, sc.look_at, sc.view_up)
    else:
        L, sp, tr = _BUILDERS[name]()
        cam = CAMERAS[name]
    assert len(L) + len(sp) + len(tr) <= MAX_PRIMS, name
    return L, sp, tr, cam


def rays(name):
    L, sp, tr, cam = scene(name)
    o, d, p1, p2 = generic_rays(L, sp, tr, seed=100 + SCENES.index(name))
    camrec = sio.make_camera(cam[0], cam[1], cam[2], 50.0, 16, 12)
    from pt_cases import primary_dirs
    pd = primary_dirs(camrec, 16, 12).reshape(-1, 3)
    po = np.tile(np.asarray(camrec["eye"], f32), (len(pd), 1))
    so, sd, s1, s2 = special_rays(name, L, sp, tr)
    o = np.concatenate([so, po, o])[:MAX_RAYS]; d = np.concatenate([sd, pd, d])[:MAX_RAYS]
    p1 = np.concatenate([s1, p1])[:MAX_RAYS]; p2 = np.concatenate([s2, p2])[:MAX_RAYS]
    ok = (p1 != p2).any(axis=1)                      # a zero-length segment has no direction
    return (np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32), np.ascontiguousarray(p1[ok], f32), np.ascontiguousarray(p2[ok], f32))


# name, scene, W, H, eye depth, spp, probe seed
RENDERS = [
    ("input-32x24-d4", "input", 32, 24, 4, 4, 11),             # four 50-degree cone lights
    ("input-16x12-d7", "input", 16, 12, 7, 8, 12),
    ("mis_test-24x18-d4", "mis_test", 24, 18, 4, 8, 13),
    ("sky-24x16-d4", "sky", 24, 16, 4, 6, 14),                 # parallel light, 25-degree cone, rough glass, eta 2.4
    ("shell-16x12-d4", "shell", 16, 12, 4, 8, 15),
    ("spheres-24x18-d4", "spheres", 24, 18, 4, 3, 16),         # camera inside the big sphere
    ("ties-20x16-d4", "ties", 20, 16, 4, 2, 17),
    ("slivers-17x13-d4", "slivers", 17, 13, 4, 5, 18),
]
BDPT = [("input", 32, 32, 2, 4), ("mis_test", 32, 32, 2, 4)]      # scene, W, H, spp, spl; depths 4 / 4, one thread
