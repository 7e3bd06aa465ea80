"""Case table of the path-tracing coverage suite: scenes, cameras and parameters at which the kernels of
csrc/pt_trace.hip, pt_shade.hip and pt_frame.hip (k_trace's quantised slab tests, hardware reciprocal, LDS tree top, node-step budget and four-wide
resume walk; k_shade; resolve, finalize, untile) and the host loop of render_pt.cpp can go wrong and the tests of
test_gpu_parity.py do not look.  A plain module: no GPU, no tests.

  geometry    _random_scene(101) moved (shifts of 1000 and 16384), scaled (1/64, 64, 4096) and stretched by one sliver to
              x = 5000 (a grid cell of the 16-bit planes is then 0.076 wide); raw camera records with exact zeros in every
              ray (d.y == 0 in the plane y = 0 and in the floor's plane, every ray exactly (0, 0, 1)); lenses of 0.3 degrees
              from 200 units away; the two floor triangles alone (a one-node tree); cornell_random_triangles(20000) far
              from the origin (a tree, not a stack, deeper than the 12 LDS levels of the resume walk); zero-area triangles and nine
              identical ones (more than a leaf holds); 64 spheres and 40 light balls
  parameters  input.txt at eye depths 1, 2, 3, 16 and 40 with and without roulette; max_delta 1, 2, 3; a box of mirrors at caps
              8, 64 and 250 (the clamp: 251 and 1000 are rendered too and must give 250's image); images of 1 x 1, 7 x 3,
              8 x 8, 9 x 65 and 1 x 257 in tiles of 8, 32 and 1024 at 1 spp and at 5 spp in passes of 2; 40 x 24 in two tiles
              for 3 and 8 ranks and 50 x 37 in 35 tiles for 5 and 7; seeds 5 + 2^32, 2^63 + 9 and 2^64 - 1; sample_offset
              2^31 - 8; the one-shot wrapper with seed 2^62; exactly 128 and 129 materials and 32 and 33 lights

Every case is `Case(name, make, dark)`; make() returns
    (L, sp, tr, cam_record, W, H, eye_depth, spp, params_kw)
where params_kw are keywords of path_tracing_amd.make_params (oracle_kw() maps them to the oracle's), and `dark` is None or
the reason why the case may be under 50 % lit.  GEOMETRY cases are walked on the host through the exported tree and
rendered as guide buffers as well; the flag matrix, the tile sizes, the rank counts and the clamped caps are tables of
their own (SHAPE_TILES, RANKS, MIRROR_CLAMPED) applied to cases of this one by test_gpu_pt_coverage.py.

Observed on the CPU oracle (oracle.pt_render, the scan, 8 threads; lit = share of pixels with a non-zero channel; closest
and shadow = rays traced; guides = coverage of tests/guides_oracle at 1 spp; tree depth = export_bvh_host's bvh_depth):
  far64             lit  89.6 %  closest  26050  shadow  9137  0.04 s  guides  99.1 %  tree depth  9
  shift-1000        lit  89.7 %  closest  26041  shadow  9132  0.02 s  guides  99.1 %  tree depth  9
  shift-16384       lit  87.7 %  closest  38104  shadow  8845  0.03 s  guides  97.6 %  tree depth  8
  scale-1/64        lit  91.4 %  closest  25826  shadow  9105  0.02 s  guides  99.0 %  tree depth  8
  scale-4096        lit  87.6 %  closest  25393  shadow  8296  0.02 s  guides  98.7 %  tree depth  8
  sliver            lit  89.6 %  closest  25995  shadow  9117  0.02 s  guides  99.1 %  tree depth  9
  camera-flat       lit  87.8 %  closest  26709  shadow  8934  0.02 s  guides 100.0 %  tree depth  8
  camera-floor      lit  72.5 %  closest  19802  shadow  5558  0.02 s  guides 100.0 %  tree depth  8
  camera-axis       lit  81.9 %  closest  26302  shadow  7841  0.02 s  guides 100.0 %  tree depth  8
  tele-axis         lit  58.7 %  closest   9444  shadow  1558  0.01 s  guides  85.3 %  tree depth  8
  tele-diagonal     lit  36.5 %  closest  10043  shadow   996  0.01 s  guides  90.9 %  tree depth  8  (dark)
  floor-only        lit  17.1 %  closest   6615  shadow   550  0.00 s  guides  14.9 %  tree depth  1  (dark)
  deep-far          lit  65.9 %  closest   4369  shadow  1385  0.70 s  guides  99.2 %  tree depth 17
  degenerate        lit  89.1 %  closest  25828  shadow  9077  0.03 s  guides  99.1 %  tree depth  9
  many-rounds       lit  72.2 %  closest  14101  shadow  3553  0.01 s  guides  92.4 %  tree depth  5
  depth-1           lit  24.9 %  closest   2975  shadow   361  0.01 s  (dark)
  depth-1-rr        lit  24.9 %  closest   2975  shadow   361  0.00 s  (dark)
  depth-2           lit  39.6 %  closest   5416  shadow   685  0.01 s  (dark)
  depth-2-rr        lit  35.5 %  closest   5232  shadow   594  0.01 s  (dark)
  depth-3           lit  47.8 %  closest   7414  shadow   927  0.01 s  (dark)
  depth-3-rr        lit  45.4 %  closest   6957  shadow   819  0.01 s  (dark)
  depth-16          lit  70.1 %  closest  16431  shadow  1977  0.01 s
  depth-16-rr       lit  62.8 %  closest  13327  shadow  1583  0.01 s
  depth-40          lit  70.5 %  closest  17520  shadow  2114  0.01 s
  depth-40-rr       lit  62.9 %  closest  13732  shadow  1621  0.01 s
  max_delta-1       lit  68.0 %  closest  14802  shadow  1824  0.01 s
  max_delta-2       lit  72.9 %  closest  16401  shadow  2018  0.01 s
  max_delta-3       lit  76.0 %  closest  17431  shadow  2127  0.01 s
  mirror-8          lit   6.2 %  closest   6864  shadow    19  0.00 s  (dark)
  mirror-64         lit  26.8 %  closest  44448  shadow    68  0.01 s  (dark)
  mirror-250        lit  44.3 %  closest  89586  shadow   137  0.02 s  (dark)
  shape-1x1-spp1    lit 100.0 %  closest      5  shadow     2  0.00 s  (dark)
  shape-1x1-spp5    lit 100.0 %  closest     24  shadow     6  0.00 s
  shape-7x3-spp1    lit  33.3 %  closest     69  shadow    11  0.00 s  (dark)
  shape-7x3-spp5    lit  85.7 %  closest    377  shadow    51  0.00 s
  shape-8x8-spp1    lit  43.8 %  closest    256  shadow    38  0.00 s  (dark)
  shape-8x8-spp5    lit  78.1 %  closest   1342  shadow   160  0.00 s
  shape-9x65-spp1   lit  37.3 %  closest   2460  shadow   245  0.00 s  (dark)
  shape-9x65-spp5   lit  83.4 %  closest  12227  shadow  1295  0.01 s
  shape-1x257-spp1  lit  42.8 %  closest   1050  shadow   110  0.00 s  (dark)
  shape-1x257-spp5  lit  83.7 %  closest   5164  shadow   546  0.00 s
  ranks-40x24       lit  54.8 %  closest   7566  shadow   905  0.01 s
  ranks-50x37       lit  54.3 %  closest  14871  shadow  1816  0.01 s
  seed-0            lit  55.9 %  closest   8982  shadow  1098  0.01 s
  seed-1            lit  50.5 %  closest   8995  shadow  1031  0.01 s
  seed-2            lit  54.0 %  closest   9016  shadow  1062  0.01 s
  offset            lit  79.7 %  closest  18078  shadow  2262  0.01 s
  wrapper-seed      lit  52.7 %  closest   8882  shadow  1061  0.01 s
  mats-128          lit  75.9 %  closest  23118  shadow  6484  0.03 s
  mats-129          lit  76.2 %  closest  23226  shadow  6529  0.03 s
  lights-32         lit  76.8 %  closest  22107  shadow  5958  0.02 s
  lights-33         lit  77.3 %  closest  22048  shadow  5912  0.02 s
In every GEOMETRY row the host walk of the exported tree gives the scan's bytes and ray counts, also with every reciprocal
moved 1 or 2 float neighbours in each of the 8 direction combinations (tests/test_pt_cases_cpu.py).  Caps 1, 2 and 3 change
193, 77 and 30 of input.txt's 1120 pixels against the default cap; the mirror box makes 8.8, 57.1 and 114.7 delta bounces
per sample at caps 8, 64 and 250, and traces fewer rays at 249 than at 250: the clamp is reached.
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
from bdpt_cases import INPUT_TXT, transform_point, transform_scene  # noqa: E402
from test_gpu_parity import _random_scene                          # noqa: E402

Case = collections.namedtuple("Case", "name make dark")

FLAG_RUSSIAN_ROULETTE = 16            # path_tracing_amd.FLAG_RUSSIAN_ROULETTE (importing the package here would load nothing, but
                                      # the table stays free of it: the flag is part of the C ABI, include/hpt.h)
SCENE_SEED = 101                      # (104 is the parallel light in the closed box: 1 % lit)
GEO_W, GEO_H, GEO_DEPTH, GEO_SPP, GEO_SEED = 48, 40, 5, 3, 7
MAX_DELTA_CAP = 250                   # take_params, csrc/hpt_api.cpp


def _cornell_cam(W, H, scale=1.0, shift=(0.0, 0.0, 0.0), eye=sio.CORNELL_EYE, look=sio.CORNELL_LOOK, fov=50.0):
    return sio.make_camera(transform_point(eye, scale, shift), transform_point(look, scale, shift), sio.CORNELL_UP, fov, W, H)


def _geo(L, sp, tr, cam, W=GEO_W, H=GEO_H, depth=GEO_DEPTH, spp=GEO_SPP, seed=GEO_SEED):
    return L, sp, tr, cam, W, H, depth, spp, dict(seed=seed)


# ---- geometry and camera: what k_trace sees ---------------------------------------------------------------------------
def moved_case(scale, shift):
    """_random_scene(101) under bdpt_cases.far_case's transform, camera too."""
    L, sp, tr = transform_scene(*_random_scene(sio, SCENE_SEED), scale, shift)
    return _geo(L, sp, tr, _cornell_cam(GEO_W, GEO_H, scale, shift))


SLIVER_X = 5000.0


def sliver_case():
    """One sliver from inside the box to x = 5000: the x extent of the tree's 16-bit grid grows from 1 to 5000, so one grid
    cell is 0.076 wide and every other box is a handful of cells in x."""
    L, sp, tr = _random_scene(sio, SCENE_SEED)
    sliver = sio._tris_from([(-0.2, -0.3, 0.4, -0.2, -0.25, 0.4, SLIVER_X, -0.3, 0.4)], [(0.8, 0.3, 0.2, 0.5, 0.0, 0.0)])
    tr = np.concatenate([tr, sliver])
    tr["id"] = np.arange(len(tr))
    return _geo(L, sp, tr, _cornell_cam(GEO_W, GEO_H))


def raw_camera_case(which):
    """Camera records no make_camera produces, with exact zeros in every ray: `flat` dy = 0 and UL.y = eye.y (d.y == 0: rays
    in the plane y = 0), `floor` the same in the floor's plane y = -0.5 (rays coplanar with the two floor triangles), `axis`
    dx = dy = 0 (every ray exactly (0, 0, 1))."""
    L, sp, tr = _random_scene(sio, SCENE_SEED)
    cam = _cornell_cam(GEO_W, GEO_H).copy()
    if which == "axis":
        cam["dx"] = 0.0
        cam["dy"] = 0.0
        cam["UL"] = (cam["eye"][0], cam["eye"][1], cam["eye"][2] + np.float32(1.0))
    else:
        y = np.float32(0.0 if which == "flat" else -0.5)
        cam["dy"] = 0.0
        cam["dx"] = (cam["dx"][0], 0.0, 0.0)
        cam["eye"] = (cam["eye"][0], y, cam["eye"][2])
        cam["UL"] = (cam["UL"][0], y, cam["UL"][2])
    return _geo(L, sp, tr, cam)


def primary_dirs(cam, W, H, jitter=0.5):
    """Directions of primary_ray (csrc/pt_device_common.h) in numpy float32, one per pixel at a fixed jitter: [H, W, 3]."""
    f = np.float32
    px = (np.arange(W, dtype=f) + f(jitter))[None, :, None]
    py = (np.arange(H, dtype=f) + f(jitter))[:, None, None]
    pos = (np.asarray(cam["UL"], f) + (np.asarray(cam["dx"], f) * px).astype(f)).astype(f)
    pos = (pos + (np.asarray(cam["dy"], f) * py).astype(f)).astype(f)
    d = (pos - np.asarray(cam["eye"], f)).astype(f)
    n2 = ((d[..., 0] * d[..., 0]).astype(f) + (d[..., 1] * d[..., 1]).astype(f)).astype(f)
    n2 = (n2 + (d[..., 2] * d[..., 2]).astype(f)).astype(f)
    return (d / np.sqrt(n2).astype(f)[..., None]).astype(f)


def tele_case(which):
    """Long lenses: nearly parallel rays from far away.  `axis` eye (0, 0, -200), fov 0.28 degrees, through the back wall
    (whose own shadow-ray crossings lie inside the 1e-3 shadow epsilon); `diagonal` eye (150, 150, -150), fov 0.3 degrees,
    looking at the middle of the box: no ray component is small and none dominates."""
    L, sp, tr = _random_scene(sio, SCENE_SEED)
    if which == "axis":
        cam = sio.make_camera((0.0, 0.0, -200.0), (0.0, 0.0, 1.0), sio.CORNELL_UP, 0.28, GEO_W, GEO_H)
    else:
        cam = sio.make_camera((150.0, 150.0, -150.0), (0.0, 0.0, 0.0), sio.CORNELL_UP, 0.3, GEO_W, GEO_H)
    return _geo(L, sp, tr, cam)


def floor_only_case():
    """The two floor triangles alone: a one-node tree whose boxes are flat in y (the degenerate-axis widening)."""
    L, sp, tr = _random_scene(sio, SCENE_SEED)
    tr = tr[:2].copy()
    assert (tr["v0"][:, 1] == -0.5).all() and (tr["v1"][:, 1] == -0.5).all() and (tr["v2"][:, 1] == -0.5).all()
    return _geo(L, sp[:0].copy(), tr, _cornell_cam(GEO_W, GEO_H))


def deep_far_case():
    """cornell_random_triangles(20000) under the far transform: a tree of 17 levels (four-wide: 9).  The tree is deeper than
    the 12 LDS levels of the resume walk, the stack is not: the host restatement of the walk (test_walk_cases_cpu.py,
    condition (c)) finds at most 12 entries, which fills the LDS levels and stores nothing to the global ones."""
    L, sp, tr = transform_scene(*sio.cornell_random_triangles(20000), 64.0, (300.0, -200.0, 500.0))
    return _geo(L, sp, tr, _cornell_cam(32, 24, 64.0, (300.0, -200.0, 500.0)), 32, 24, 3, 2)


N_IDENTICAL = 9


def degenerate_case():
    """_random_scene(101) plus zero-area triangles (three collinear points, two equal vertices, three equal vertices; their
    boxes are flat or points) and a block of 9 identical triangles, more than a leaf of 8 holds: the builder has to cut a
    set it cannot separate, and the scan's first-of-equals rule decides among the copies."""
    L, sp, tr = _random_scene(sio, SCENE_SEED)
    zero = [(-0.3, -0.2, 0.3, 0.0, 0.0, 0.4, 0.3, 0.2, 0.5),              # collinear
            (0.1, -0.3, 0.2, 0.1, -0.3, 0.2, 0.3, 0.1, 0.6),              # v0 == v1
            (-0.2, 0.25, 0.5, -0.2, 0.25, 0.5, -0.2, 0.25, 0.5)]          # a point
    same = [(-0.35, -0.35, 0.6, 0.05, -0.35, 0.7, -0.15, 0.1, 0.65)] * N_IDENTICAL
    mats = [(0.9, 0.1, 0.1, 1.0, 0.0, 0.0)] * 3 + [(0.1 + 0.1 * k, 0.9 - 0.1 * k, 0.3, 1.0, 0.0, 0.0) for k in range(N_IDENTICAL)]
    tr = np.concatenate([tr, sio._tris_from(zero + same, mats)])
    tr["id"] = np.arange(len(tr))
    return _geo(L, sp, tr, _cornell_cam(GEO_W, GEO_H))


N_SPHERES, N_BALL_LIGHTS = 64, 40


def many_rounds_case():
    """The Cornell walls, 64 spheres of mixed material and 40 lights: the sphere loops of trace_chunk run 104 (closest hit:
    spheres and light balls) and 64 (shadow) long."""
    rng = np.random.default_rng(64)
    palette = [(0.7, 0.7, 0.7, 1.0, 0.0, 0.0), (0.8, 0.3, 0.2, 0.5, 0.0, 0.0), (0.9, 0.8, 0.3, 0.3, 0.9, 0.0),
               (0.95, 0.95, 0.95, 0.0, 1.0, 0.0), (1.0, 1.0, 1.0, 0.0, 0.0, 1.5), (0.2, 0.6, 0.9, 0.05, 0.0, 0.0)]
    tr = sio._tris_from([t for _, tl in sio._CORNELL_WALLS for t in tl], [m6 for m6, tl in sio._CORNELL_WALLS for _ in tl])
    sp = np.zeros(N_SPHERES, SPHERE)
    for k in range(N_SPHERES):
        m = palette[k % len(palette)]
        sp[k]["center"] = rng.uniform([-0.42, -0.45, 0.0], [0.42, 0.1, 0.9]); sp[k]["r"] = rng.uniform(0.03, 0.07)
        sp[k]["mtl"]["base_color"] = m[0:3]; sp[k]["mtl"]["roughness"] = m[3]
        sp[k]["mtl"]["metallic"] = m[4]; sp[k]["mtl"]["eta"] = m[5]; sp[k]["id"] = k
    return _geo(_lights(rng, N_BALL_LIGHTS), sp, tr, _cornell_cam(GEO_W, GEO_H), depth=4, spp=2)


def _lights(rng, n):
    """The light generator of test_many_materials_and_lights_beyond_the_lds_staging: ball, cone and parallel lights."""
    lights = []
    for k in range(n):
        pos = tuple(rng.uniform([-0.4, 0.1, -0.1], [0.4, 0.45, 0.9]))
        if k % 5 == 4:
            lights.append(sio._one_light(pos, (0.1, -1.0, 0.2), (0.05, 0.05, 0.05), 0.0, 1, 0.03))
        else:
            lights.append(sio._one_light(pos, (0.0, -1.0, 0.0), tuple(rng.uniform(0.02, 0.1, size=3)), 180.0 if k % 2 else 50.0, 0, 0.03))
    return np.concatenate(lights)


# ---- parameters: what k_shade, the host loop, resolve, finalize and untile see ----------------------------------------
def _input(W, H):
    sc = sio.load_scene(INPUT_TXT)
    L, sp, tr = sio.flatten_for_pt(sc)
    return L, sp, tr, sio.camera_for(sc, W, H)


DEPTHS = [1, 2, 3, 16, 40]


def depth_case(depth, roulette):
    L, sp, tr, cam = _input(40, 28)
    return L, sp, tr, cam, 40, 28, depth, 2, dict(seed=8, flags=FLAG_RUSSIAN_ROULETTE if roulette else 0)


MAX_DELTAS = [1, 2, 3]


def max_delta_case(max_delta):
    """max_delta 0 = the default cap (64); 8 changes nothing on input.txt."""
    L, sp, tr, cam = _input(40, 28)
    return L, sp, tr, cam, 40, 28, 4, 4, dict(seed=8, max_delta=max_delta)


MIRROR_DELTAS = [8, 64, 250]
MIRROR_CLAMPED = [251, 1000]


def mirror_box_case(max_delta):
    """cornell_diffuse's box with its 12 walls perfect mirrors (the two small boxes stay diffuse), a light ball of r 0.03,
    looked into off-axis: paths bounce between the walls until the cap ends them."""
    L, sp, tr = sio.cornell_diffuse()
    tr = tr[:24].copy()
    tr["mtl"]["base_color"][:12] = 1.0
    tr["mtl"]["roughness"][:12] = 0.0
    tr["mtl"]["metallic"][:12] = 1.0
    tr["mtl"]["type"][:12] = 2
    L = L.copy()
    L["light_ball"]["r"] = 0.03
    cam = sio.make_camera((0.0, 0.0, -1.0), (0.13, 0.07, 1.0), sio.CORNELL_UP, 50.0, 24, 16)
    return L, sp, tr, cam, 24, 16, 3, 2, dict(seed=5, max_delta=max_delta)


SHAPES = [(1, 1), (7, 3), (8, 8), (9, 65), (1, 257)]
SHAPE_TILES = [8, 32, 1024]
SHAPE_SPP = [(1, 0), (5, 2)]                       # (spp, samples_per_pass): 5 = 2 + 2 + 1, a one-sample last pass on one pipeline


def shape_case(W, H, spp, samples_per_pass):
    L, sp, tr, cam = _input(W, H)
    return L, sp, tr, cam, W, H, 4, spp, dict(seed=2, samples_per_pass=samples_per_pass)      # seed 2: the 1 x 1 image is lit at 1 spp


RANKS = {"ranks-40x24": (40, 24, 32, (3, 8)),      # two tiles: ranks 2.. own no pixel
         "ranks-50x37": (50, 37, 8, (5, 7))}       # 7 x 5 = 35 tiles


def rank_case(name):
    W, H = RANKS[name][:2]
    L, sp, tr, cam = _input(W, H)
    return L, sp, tr, cam, W, H, 4, 2, dict(seed=15)


HIGH_SEEDS = [5 + 2**32, 2**63 + 9, 2**64 - 1]
BIG_OFFSET = 2**31 - 8
WRAPPER_SEED = 2**62


def seed_case(seed, sample_offset=0, spp=2):
    L, sp, tr, cam = _input(40, 28)
    return L, sp, tr, cam, 40, 28, 4, spp, dict(seed=seed, sample_offset=sample_offset)


STAGING = [("mats", 128), ("mats", 129), ("lights", 32), ("lights", 33)]     # kLdsMats, kLdsLights of k_shade: the last that fits, the first that does not
N_WALL_MATS = 6


def staging_case(what, count):
    """The generator of test_many_materials_and_lights_beyond_the_lds_staging at 64 x 48: every added triangle its own
    material, so `count` materials are the 6 of the walls and count - 6 triangles (with 8 lights); or 60 triangles and
    `count` lights."""
    n = count - N_WALL_MATS if what == "mats" else 60
    rng = np.random.default_rng(77)
    rows = [t for _, tl in sio._CORNELL_WALLS for t in tl]
    mats = [m6 for m6, tl in sio._CORNELL_WALLS for _ in tl]
    c = rng.uniform([-0.4, -0.4, -0.1], [0.4, 0.4, 0.9], size=(n, 1, 3))
    v = (c + rng.uniform(-0.1, 0.1, size=(n, 3, 3))).reshape(n, 9)
    rows += [tuple(r) for r in v.astype(np.float32)]
    for k in range(n):
        kind = k % 4
        base = tuple(rng.uniform(0.1, 1.0, size=3))
        mats.append(base + ((1.0, 0.0, 0.0) if kind == 0 else (float(rng.uniform(0.2, 0.8)), 0.0, 0.0) if kind == 1
                            else (float(rng.uniform(0.1, 0.5)), 0.9, 0.0) if kind == 2 else (0.0, 1.0, 0.0)))
    tr = sio._tris_from(rows, mats)
    L = _lights(rng, count if what == "lights" else 8)
    if what == "mats":
        L["illum"] *= np.float32(4.0)                  # 8 lights instead of 40
    return L, np.zeros(0, SPHERE), tr, _cornell_cam(64, 48), 64, 48, 4, 2, dict(seed=5)


def n_materials(sp, tr):
    """Distinct 28-byte material records: what scene_build.cpp interns and hpt_stats.n_materials reports."""
    return len({m.tobytes() for a in (sp, tr) for m in a["mtl"]})


# ---- the table -------------------------------------------------------------------------------------------------------
def _bind(fn, *a):
    return lambda: fn(*a)


FAR_SHIFT = (300.0, -200.0, 500.0)
GEOMETRY = [
    Case("far64", _bind(moved_case, 64.0, FAR_SHIFT), None),
    Case("shift-1000", _bind(moved_case, 1.0, (1000.0, -1000.0, 2000.0)), None),
    Case("shift-16384", _bind(moved_case, 1.0, (16384.0, -16384.0, 16384.0)), None),
    Case("scale-1/64", _bind(moved_case, 1.0 / 64.0, (0.0, 0.0, 0.0)), None),
    Case("scale-4096", _bind(moved_case, 4096.0, (0.0, 0.0, 0.0)), None),
    Case("sliver", sliver_case, None),
    Case("camera-flat", _bind(raw_camera_case, "flat"), None),
    Case("camera-floor", _bind(raw_camera_case, "floor"), None),
    Case("camera-axis", _bind(raw_camera_case, "axis"), None),
    Case("tele-axis", _bind(tele_case, "axis"), None),
    Case("tele-diagonal", _bind(tele_case, "diagonal"), "a 0.3-degree lens from outside the box: the views onto the outsides of walls, which no light reaches, stay black"),
    Case("floor-only", floor_only_case, "two triangles under an open sky: six of seven primary rays hit nothing"),
    Case("deep-far", deep_far_case, None),
    Case("degenerate", degenerate_case, None),
    Case("many-rounds", many_rounds_case, None),
]
# cases whose first non-delta hit covers the image: render_guides at 1 spp is then a per-ray view of k_trace
GUIDES = [c.name for c in GEOMETRY if c.name != "floor-only"]
ZERO_COMPONENT = {"camera-flat": "y", "camera-floor": "y", "camera-axis": "xy"}

_SHALLOW = "input.txt at 2 spp: within three bounces its four cone lights reach under half of the pixels (depth 16: 70 %)"
_MIRRORS = "a box of mirrors: a sample is lit only where its path meets the r 0.03 light ball or a small diffuse box before the cap"
_ONE_SAMPLE = "one sample per pixel of input.txt lights about a third of the pixels (five samples: over 80 %)"
PARAMETERS = (
    [Case("depth-%d%s" % (d, "-rr" if rr else ""), _bind(depth_case, d, rr), _SHALLOW if d <= 3 else None) for d in DEPTHS for rr in (False, True)]
    + [Case("max_delta-%d" % m, _bind(max_delta_case, m), None) for m in MAX_DELTAS]
    + [Case("mirror-%d" % m, _bind(mirror_box_case, m), _MIRRORS) for m in MIRROR_DELTAS]
    + [Case("shape-%dx%d-spp%d" % (W, H, spp), _bind(shape_case, W, H, spp, spass), _ONE_SAMPLE if spp == 1 else None)
       for W, H in SHAPES for spp, spass in SHAPE_SPP]
    + [Case(name, _bind(rank_case, name), None) for name in RANKS]
    + [Case("seed-%d" % k, _bind(seed_case, s), None) for k, s in enumerate(HIGH_SEEDS)]
    + [Case("offset", _bind(seed_case, 8, BIG_OFFSET, 4), None)]
    + [Case("wrapper-seed", _bind(seed_case, WRAPPER_SEED), None)]
    + [Case("%s-%d" % s, _bind(staging_case, *s), None) for s in STAGING]
)
CASES = GEOMETRY + PARAMETERS
DARK = (["tele-diagonal", "floor-only"] + ["depth-%d%s" % (d, rr) for d in (1, 2, 3) for rr in ("", "-rr")]
        + ["mirror-%d" % m for m in MIRROR_DELTAS] + ["shape-%dx%d-spp1" % s for s in SHAPES])
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

_REFERENCE = {}
_TREES = {}


def oracle_kw(params_kw):
    """oracle.pt_render's keywords for a case's make_params keywords (the library clamps max_delta to 250)."""
    kw = dict(seed=params_kw.get("seed", 1), sample_offset=params_kw.get("sample_offset", 0),
              russian_roulette=bool(params_kw.get("flags", 0) & FLAG_RUSSIAN_ROULETTE))
    if params_kw.get("max_delta", 0) > 0:
        kw["max_delta"] = min(params_kw["max_delta"], MAX_DELTA_CAP)
    return kw


def oracle_render(oracle_mod, args, **extra):
    """(image, stats) of the CPU oracle -- the scan unless `bvh` is handed over -- for the 9-tuple a case's make() returns."""
    L, sp, tr, cam, W, H, depth, spp, kw = args
    return oracle_mod.pt_render(L, sp, tr, cam, W, H, depth, spp, **dict(oracle_kw(kw), **extra))


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
