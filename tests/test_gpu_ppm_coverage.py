"""Photon mapping and progressive photon mapping on the MI355X against the CPU restatements, where the kernels can go
wrong and the first suites (test_gpu_ppm.py, test_gpu_sppm.py) do not look: the photon grid's radix sort on each of
rocPRIM's size-selected algorithms up to the benchmark's 16 Mi deposit slots; random scenes with every material class
and the delta / deposit thresholds exactly; edge scenes, image shapes, tiles, depths, radii and bounds, including
cells far from the origin where the SPPM cull's margin is tightest and cell coordinates are clamped.

Every comparison is bytes of the image, the five counts and, with FLAG_COUNT_WORK, the pairs examined and accepted
(for PPM also their median and maximum per hit point); SPPM also compares the per-pixel R2 and N."""
import os
import re

import numpy as np
import pytest

import ppm_oracle
import sppm_oracle
from test_gpu_parity import _random_scene
from test_gpu_ppm import _load

pytestmark = pytest.mark.gpu

COUNTS = ("photons", "photon_rays", "deposits", "hit_points", "direct_pixels")


@pytest.fixture(scope="module")
def olib(tmp_path_factory):
    """One build of both oracles (sppm_oracle.cpp includes ppm_oracle.cpp)."""
    return sppm_oracle.build(tmp_path_factory.mktemp("ppm_cov_oracle"))


def _bounds(sp, tr, scene_min, scene_max):
    mn, mx = ppm_oracle.scene_bounds(np.ascontiguousarray(sp), np.ascontiguousarray(tr))
    return (mn if scene_min is None else np.asarray(scene_min, np.float32)), (mx if scene_max is None else np.asarray(scene_max, np.float32))


def ppm_parity(hpt, lib, L, sp, tr, cam, W, H, eye_depth=4, light_depth=4, spp=1, spl=64, radius=0.05, seed=11,
               sample_offset=0, max_delta=0, tile=0, scene_min=None, scene_max=None):
    """render_ppm with COUNT_WORK equals the PPM oracle: image bytes, counts, pairs and their per-hit-point spread."""
    with hpt.Scene(L, sp, tr) as s:
        p = hpt.make_params(seed=seed, sample_offset=sample_offset, max_delta=max_delta, tile=tile, flags=hpt.FLAG_COUNT_WORK)
        img = s.render_ppm(cam, W, H, eye_depth, light_depth, spp, spl, radius, p, scene_min=scene_min, scene_max=scene_max)
        st = s.ppm_stats()
    ref, rst = ppm_oracle.render(lib, L, sp, tr, cam, W, H, eye_depth, light_depth, spp, spl, radius, seed=seed,
                                 sample_offset=sample_offset, max_delta=max_delta, scene_min=scene_min, scene_max=scene_max,
                                 want_work=True)
    for k in COUNTS + ppm_oracle.WORK:
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert img.tobytes() == ref.tobytes()
    return img, st


def sppm_parity(hpt, lib, L, sp, tr, cam, W, H, calls=(1, 2), eye_depth=4, light_depth=4, spl=64, radius=0.05, alpha=0.7,
                seed=11, sample_offset=0, max_delta=0, tile=0, scene_min=None, scene_max=None, cull_check=False):
    """Scene.sppm with COUNT_WORK on every call equals the SPPM oracle call for call: image bytes, the seven counts,
    and R2 / N at the end.  cull_check: the oracle without the cull gives the same bytes and examines no fewer pairs."""
    ref = sppm_oracle.State(lib, L, sp, tr, cam, W, H, eye_depth, light_depth, spl, radius, alpha, seed, sample_offset,
                            max_delta, scene_min, scene_max)
    full = sppm_oracle.State(lib, L, sp, tr, cam, W, H, eye_depth, light_depth, spl, radius, alpha, seed, sample_offset,
                             max_delta, scene_min, scene_max, cull=False) if cull_check else None
    with hpt.Scene(L, sp, tr) as s:
        p = hpt.make_params(seed=seed, sample_offset=sample_offset, max_delta=max_delta, tile=tile)
        with s.sppm(cam, W, H, eye_depth, light_depth, spl, radius, alpha, p, scene_min=scene_min, scene_max=scene_max) as z:
            for it, n in enumerate(calls):
                img = z.render(n, flags=hpt.FLAG_COUNT_WORK)
                st = s.ppm_stats()
                rimg, rst = ref.render(n)
                for k in sppm_oracle.STATS:
                    assert st[k] == rst[k], (it, k, st[k], rst[k])
                assert img.tobytes() == rimg.tobytes(), it
                if full is not None:
                    fimg, fst = full.render(n)
                    assert fimg.tobytes() == rimg.tobytes(), it
                    assert fst["accepted"] == rst["accepted"] and rst["candidates"] <= fst["candidates"], (it, rst, fst)
            state = z.state()
    assert state["passes"] == sum(calls)
    assert state["radius2"].tobytes() == ref.r2.tobytes()
    assert state["photons"].tobytes() == ref.n.tobytes()
    if full is not None:
        assert full.r2.tobytes() == ref.r2.tobytes() and full.n.tobytes() == ref.n.tobytes()
    return img, rst


# ---- A. the grid's sort on each of rocPRIM's algorithms, up to the benchmark's size ----------------------------------
def _rocprim_sort_thresholds():
    """(single-block items, merge sort limit) of rocprim::radix_sort_pairs with the default config, read from the
    installed headers (radix_sort_impl: one block up to block_size * items_per_thread of the small block sort, merge
    sort up to merge_sort_limit, onesweep above)."""
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include", "rocprim", "device")
    impl = open(os.path.join(inc, "device_radix_sort.hpp")).read()
    conf = open(os.path.join(inc, "device_radix_sort_config.hpp")).read()
    blk = re.search(r"kernel_config<rocprim::min\((\d+)u,\s*default_radix_sort_block_sort_config::block_size\),\s*"
                    r"rocprim::min\((\d+)u,\s*default_radix_sort_block_sort_config::items_per_thread\)>", impl)
    lim = re.search(r"size_t\s+MergeSortLimit\s*=\s*(\d+)\s*\*\s*(\d+)\s*>", conf)
    assert blk and lim, "rocPRIM's radix sort dispatch changed: re-derive the cases of SORT_CASES"
    assert "single_sort_items_per_block" in impl and "merge_sort_limit" in impl
    return int(blk.group(1)) * int(blk.group(2)), int(lim.group(1)) * int(lim.group(2))


SORT_CASES = [  # light_depth, spl on input.txt (4 lights): n_slots = 4 * spl * light_depth
    (1, 256), (1, 257), (4, 65536), (4, 65537), (4, 262144), (4, 300000), (4, 1000000)]


def test_sort_cases_straddle_rocprims_thresholds():
    """The cases below sit on both sides of each algorithm switch of the installed rocPRIM (single block <= 1024 items
    at most, merge sort <= 1 Mi); a ROCm whose thresholds moved fails here instead of silently losing coverage."""
    single, merge = _rocprim_sort_thresholds()
    assert (single, merge) == (1024, 1 << 20)
    slots = [4 * spl * ld for ld, spl in SORT_CASES]
    assert slots[0] == single and slots[1] == single + 4
    assert slots[2] == merge and slots[3] == merge + 16
    assert slots[-1] == 16_000_000 > 1 << 23       # scripts/bench_ppm.py: 4 lights x 10^6 photons x depth 4


@pytest.mark.parametrize("ld,spl", SORT_CASES, ids=["slots%d" % (4 * spl * ld) for ld, spl in SORT_CASES])
def test_ppm_grid_sort_sizes_match_the_oracle(hpt, sio, olib, ld, spl):
    """Odd-sized image, input.txt, bench density at the largest size (a grid of 2^25 buckets, sentinel key in bit 25;
    thousands of candidates per hit point): bytes, counts, pairs and their median / maximum per hit point."""
    W, H = 72, 56
    L, sp, tr, cam = _load(sio, "input", W, H)
    n = 4 * spl * ld
    buckets = 1024
    while buckets < 2 * n:
        buckets *= 2
    img, st = ppm_parity(hpt, olib, L, sp, tr, cam, W, H, light_depth=ld, spl=spl, seed=31)
    assert st["grid_buckets"] == buckets
    assert st["deposits"] > n // 4 and st["accepted"] > 0 and img.max() > 0
    if n > 1 << 23:
        assert st["cand_median"] > 1000


@pytest.mark.parametrize("spl", [300000, 1000000], ids=["slots4800000", "slots16000000"])
def test_sppm_onesweep_size_matches_the_oracle(hpt, sio, olib, spl):
    """Three SPPM passes (alpha 0.7) on the onesweep path: 2^24 buckets, and the benchmark's 2^25."""
    W, H = 72, 56
    L, sp, tr, cam = _load(sio, "input", W, H)
    _, rst = sppm_parity(hpt, olib, L, sp, tr, cam, W, H, calls=(1, 2), spl=spl, alpha=0.7, seed=32)
    assert rst["accepted"] > 0


# ---- B. random scenes with every material class and the thresholds themselves ------------------------------------
THRESHOLD_MATS = [              # r, g, b, roughness, metallic, eta
    (0.9, 0.9, 0.9, 0.001, 1.0, 0.0),      # rough enough to be non-delta; no deposit (metallic >= 0.99, roughness <= 0.01)
    (0.9, 0.9, 0.9, 0.001, 0.0, 1.5),      # non-delta rough dielectric at the delta threshold
    (0.8, 0.7, 0.6, 0.01, 1.0, 0.0),       # roughness at the deposit threshold: no deposit
    (0.8, 0.8, 0.8, 0.01, 0.0, 0.0),       # opaque dielectric, roughness 0.01: deposit
    (0.9, 0.9, 0.9, 0.0, 0.01, 1.5),       # metallic at the glass threshold: non-delta, no deposit
    (0.9, 0.8, 0.7, 0.0, 0.99, 0.0),       # metallic at the mirror threshold: non-delta, no deposit
    (0.9, 0.9, 0.9, 0.005, 0.995, 0.0),    # near-mirror: non-delta, no deposit
    (0.7, 0.9, 0.7, 0.3, 0.0, 1.5),        # rough dielectric: non-delta, no deposit
    (1.0, 1.0, 1.0, 0.0, 0.0, 1.5),        # smooth glass: delta
    (0.95, 0.95, 0.95, 0.0, 1.0, 0.0),     # mirror: delta
]


def _ppm_random_scene(sio, seed, nl):
    """_random_scene(seed) plus two triangles and a sphere of every THRESHOLD_MATS entry (glass and mirrors stacked
    in chains), and nl lights of mixed kinds (spot, wide cone, parallel) in place of its own; a radius per seed."""
    from path_tracing_amd.layouts import SPHERE
    _, sp0, tr0 = _random_scene(sio, seed)
    rng = np.random.default_rng(seed + 7000)
    rows, mats = [], []
    for m in THRESHOLD_MATS:
        for _ in range(2):
            c = rng.uniform([-0.35, -0.35, 0.1], [0.35, 0.35, 0.7])
            v = c + rng.uniform(-0.18, 0.18, size=(3, 3))
            rows.append(tuple(v.reshape(9).astype(np.float32))); mats.append(m)
    for k in range(3):                                   # a chain: mirror, glass, mirror facing each other
        z = 0.3 + 0.15 * k
        rows.append((-0.3, -0.3, z, 0.3, -0.3, z + 0.02, 0.0, 0.3, z)); mats.append(THRESHOLD_MATS[9 if k != 1 else 8])
    tr = np.concatenate([tr0, sio._tris_from(rows, mats)])
    sp = np.zeros(len(THRESHOLD_MATS), SPHERE)
    for k, m in enumerate(THRESHOLD_MATS):
        sp[k]["center"] = rng.uniform([-0.35, -0.35, 0.1], [0.35, 0.35, 0.8]); sp[k]["r"] = rng.uniform(0.04, 0.09)
        sp[k]["mtl"]["base_color"] = m[0:3]; sp[k]["mtl"]["roughness"] = m[3]
        sp[k]["mtl"]["metallic"] = m[4]; sp[k]["mtl"]["eta"] = m[5]; sp[k]["id"] = len(sp0) + k
    sp = np.concatenate([sp0, sp])
    lights = []
    for k in range(nl):
        kind = k % 3
        pos = tuple(rng.uniform([-0.35, 0.2, 0.0], [0.35, 0.45, 0.8]))
        if kind == 2:
            lights.append(sio._one_light(pos, tuple(rng.uniform([-0.4, -1.0, -0.3], [0.4, -0.6, 0.3])), (0.5, 0.5, 0.5), 0.0, 1, 0.03))
        else:
            d = tuple(rng.uniform([-0.5, -1.0, -0.5], [0.5, -0.5, 0.5]))
            lights.append(sio._one_light(pos, d, tuple(rng.uniform(0.3, 1.2, size=3)), 170.0 if kind == 0 else 35.0, 0,
                                         float(rng.uniform(0.02, 0.06))))
    radius = float(rng.uniform(0.03, 0.15))
    return np.concatenate(lights), sp, tr, radius


PPM_SEEDS = [(301, 1), (302, 3), (303, 5), (304, 36), (305, 3), (306, 5)]


@pytest.mark.parametrize("seed,nl", PPM_SEEDS, ids=["seed%d_nl%d" % c for c in PPM_SEEDS])
def test_random_scenes_ppm_match_the_oracle(hpt, sio, olib, seed, nl):
    L, sp, tr, radius = _ppm_random_scene(sio, seed, nl)
    W, H = 48, 40
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)
    img, st = ppm_parity(hpt, olib, L, sp, tr, cam, W, H, eye_depth=5, light_depth=4, spp=2, spl=max(64, 1024 // nl),
                         radius=radius, seed=seed)
    assert st["hit_points"] > 0 and st["deposits"] > 0 and st["accepted"] > 0


@pytest.mark.parametrize("seed,nl", [(311, 3), (312, 36), (313, 1)], ids=["seed311_nl3", "seed312_nl36", "seed313_nl1"])
def test_random_scenes_sppm_match_the_oracle(hpt, sio, olib, seed, nl):
    L, sp, tr, radius = _ppm_random_scene(sio, seed, nl)
    W, H = 40, 32
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)
    _, rst = sppm_parity(hpt, olib, L, sp, tr, cam, W, H, calls=(1, 2), eye_depth=5, spl=max(64, 1024 // nl), radius=radius,
                         alpha=0.6, seed=seed)
    assert rst["accepted"] > 0


# ---- C. edge scenes and parameters -------------------------------------------------------------------------------
def _edge_scene(sio, case):
    from path_tracing_amd.layouts import LIGHT, SPHERE, TRIANGLE
    sc = sio.load_scene(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes", "input.txt"))
    L0, sp0, tr0 = sio.flatten_for_pt(sc)
    L, sp, tr = np.zeros(0, LIGHT), np.zeros(0, SPHERE), np.zeros(0, TRIANGLE)
    if case == "lights_only":
        L = L0
    elif case == "one_triangle":
        L, tr = L0, tr0[6:7]
    elif case == "no_lights":
        sp, tr = sp0, tr0
    elif case == "spheres_only":
        L, sp = L0, sp0
    elif case == "delta_only":                          # every surface a mirror or smooth glass: no hit point, no deposit
        L, sp, tr = L0, sp0.copy(), tr0.copy()
        tr["mtl"]["roughness"] = 0.0; tr["mtl"]["metallic"] = 1.0; tr["mtl"]["eta"] = 0.0
        sp["mtl"]["roughness"] = 0.0; sp["mtl"]["metallic"] = 0.0; sp["mtl"]["eta"] = 1.5
    return L, sp, tr


@pytest.mark.parametrize("case", ["empty", "lights_only", "no_lights", "spheres_only", "one_triangle", "delta_only"])
def test_edge_scenes(hpt, sio, olib, case):
    L, sp, tr = _edge_scene(sio, case)
    W, H = 40, 24
    cam = sio.make_camera((0, 0, -1), (0, 0, 1), (0, 1, 0), 50.0, W, H)
    img, st = ppm_parity(hpt, olib, L, sp, tr, cam, W, H, spp=2, spl=256, seed=4)
    simg, sst = sppm_parity(hpt, olib, L, sp, tr, cam, W, H, calls=(2,), spl=256, seed=4)
    mn, mx = _bounds(sp, tr, None, None)
    one = hpt.ppm_render_wrapper(L, sp, tr, cam, W, H, mn, mx, 4, 256, 4, 1, seed=4)
    ref, _ = ppm_oracle.render(olib, L, sp, tr, cam, W, H, 4, 4, 1, 256, 0.05, seed=4, scene_min=mn, scene_max=mx)
    hpt.wrapper_cache_clear()
    assert one.tobytes() == ref.tobytes()
    if case in ("empty", "no_lights"):
        assert not img.any() and not simg.any()
    if case in ("empty", "lights_only", "delta_only"):
        assert st["deposits"] == 0 and st["hit_points"] == 0 and st["candidates"] == 0
    if case == "delta_only":
        assert st["photon_rays"] > st["photons"]        # photons bounced off the mirrors before they left
    if case == "spheres_only":
        assert st["accepted"] > 0


EDGE_PARAMS = [  # id, W, H, keyword arguments of ppm_parity / sppm_parity
    ("spl0", 37, 23, dict(spl=0)),
    ("img1x1", 1, 1, dict()),
    ("img1x67", 1, 67, dict()),
    ("img67x1", 67, 1, dict()),
    ("img37x23", 37, 23, dict()),
    ("tile8", 37, 23, dict(tile=8)),
    ("tile40", 67, 45, dict(tile=40)),
    ("tile1024", 37, 23, dict(tile=1024)),
    ("eye_depth1", 37, 23, dict(eye_depth=1)),
    ("light_depth1", 37, 23, dict(light_depth=1)),
    ("light_depth255", 37, 23, dict(light_depth=255, spl=16)),
    ("max_delta1", 37, 23, dict(max_delta=1)),
    ("max_delta250", 37, 23, dict(max_delta=250)),
    ("radius_inf", 37, 23, dict(radius=float("inf"))),
    ("radius_3", 37, 23, dict(radius=3.0)),
    ("radius_1e-4", 37, 23, dict(radius=1e-4, spl=4096)),
    ("radius_1e-10", 37, 23, dict(radius=1e-10)),
    ("sample_offset_2p31m2", 37, 23, dict(sample_offset=2 ** 31 - 2)),
]


@pytest.mark.parametrize("W,H,kw", [c[1:] for c in EDGE_PARAMS], ids=[c[0] for c in EDGE_PARAMS])
def test_edge_parameters(hpt, sio, olib, W, H, kw):
    """input.txt with one parameter at an edge: PPM over three passes, SPPM over 1 + 2 passes (alpha 0.7)."""
    L, sp, tr, cam = _load(sio, "input", W, H)
    kw = dict(kw)
    kw.setdefault("spl", 256)
    img, st = ppm_parity(hpt, olib, L, sp, tr, cam, W, H, spp=3, seed=41, **kw)
    sppm_parity(hpt, olib, L, sp, tr, cam, W, H, calls=(1, 2), seed=41, **kw)
    if kw.get("spl") == 0:
        assert st["deposits"] == 0 and st["photons"] == 0
    if kw.get("radius") == 3.0:                         # one cell holds the scene: every hit point examines every deposit
        assert st["cand_median"] == st["cand_max"] > 0.5 * st["deposits"] / 3


@pytest.mark.parametrize("radius", [0.0, -1.0, float("nan")], ids=["zero", "negative", "nan"])
def test_radius_defaults_to_0_05(hpt, sio, radius):
    L, sp, tr, cam = _load(sio, "input", 37, 23)
    p = hpt.make_params(seed=43)
    with hpt.Scene(L, sp, tr) as s:
        ref = s.render_ppm(cam, 37, 23, 4, 4, 2, 256, 0.05, p)
        got = s.render_ppm(cam, 37, 23, 4, 4, 2, 256, radius, p)
        with s.sppm(cam, 37, 23, 4, 4, 256, 0.05, 0.7, p) as a, s.sppm(cam, 37, 23, 4, 4, 256, radius, 0.7, p) as b:
            sa, sb = a.render(2), b.render(2)
            ra, rb = a.state()["radius2"], b.state()["radius2"]
    assert ref.max() > 0
    assert got.tobytes() == ref.tobytes() and sb.tobytes() == sa.tobytes() and rb.tobytes() == ra.tobytes()


def _far_bounds(sp, tr, radius, u, above):
    """Bounds that put every point's grid coordinate u = (p - smin) / radius near +u (smin below the scene) or -u
    (smin above it: negative cells)."""
    mn, mx = ppm_oracle.scene_bounds(np.ascontiguousarray(sp), np.ascontiguousarray(tr))
    off = np.float32(u * radius)
    return ((mx + off) if above else (mn - off)).astype(np.float32), mx


FAR = [  # id, |u| target, smin above the scene
    ("u2p19_below", 600_000, False), ("u2p19_above", 600_000, True),
    ("u2p20_below", 1_500_000, False), ("u2p20_above", 1_500_000, True),
]


@pytest.mark.parametrize("u,above", [c[1:] for c in FAR], ids=[c[0] for c in FAR])
def test_far_bounds_ppm_and_sppm_cull(hpt, sio, olib, u, above):
    """Cells near 2^19 .. 2^21 from the bounds' corner, on both sides: u is rounded to 1/16 .. 1/4 of a cell, which the
    SPPM cull's margin must absorb.  Six SPPM passes at alpha 0.6 shrink the radii so the cull skips cells; the
    oracle without the cull gives the same bytes, R2 and N."""
    W, H = 48, 40
    L, sp, tr, cam = _load(sio, "input", W, H)
    mn, mx = _far_bounds(sp, tr, 0.05, u, above)
    _, st = ppm_parity(hpt, olib, L, sp, tr, cam, W, H, spp=2, spl=2048, scene_min=mn, scene_max=mx, seed=51)
    assert st["accepted"] > 0
    sppm_parity(hpt, olib, L, sp, tr, cam, W, H, calls=(2, 4), spl=8192, alpha=0.6, seed=52, scene_min=mn, scene_max=mx,
                cull_check=True)


def test_tiny_radius_clamps_cells_and_sppm_agrees_without_the_cull(hpt, sio, olib):
    """radius 1e-10: |u| passes 2^31 for most points, where the cell coordinate is clamped to 2^30."""
    W, H = 37, 23
    L, sp, tr, cam = _load(sio, "input", W, H)
    sppm_parity(hpt, olib, L, sp, tr, cam, W, H, calls=(1, 2), spl=256, radius=1e-10, seed=53, cull_check=True)


def test_sppm_small_alpha_and_many_passes(hpt, sio, olib):
    L, sp, tr, cam = _load(sio, "input", 21, 17)
    sppm_parity(hpt, olib, L, sp, tr, cam, 21, 17, calls=(1, 2), spl=256, alpha=1e-3, seed=61)
    sppm_parity(hpt, olib, L, sp, tr, cam, 21, 17, calls=(1, 15, 16), spl=128, alpha=0.7, seed=62)


def test_sppm_alpha_one_is_the_mean_of_ppm_passes(hpt, sio):
    """SPPM with alpha = 1 keeps R2 and sums the flux, so over K passes it is render_ppm with spp = K wherever neither
    clamp at 15 engages.  Not bytes: PPM clamps each pass's radiance and then averages the passes (sum of per-pass
    quotients), SPPM clamps the average (quotient of the summed flux), so the two round differently."""
    W, H, K = 48, 40, 4
    L, sp, tr, cam = _load(sio, "input", W, H)
    with hpt.Scene(L, sp, tr) as s:
        p = hpt.make_params(seed=71)
        ppm = s.render_ppm(cam, W, H, 4, 4, K, 512, 0.06, p)
        passes = [s.render_ppm(cam, W, H, 4, 4, 1, 512, 0.06, hpt.make_params(seed=71, sample_offset=k)) for k in range(K)]
        with s.sppm(cam, W, H, 4, 4, 512, 0.06, 1.0, p) as z:
            sppm = z.render(K)
            r2 = z.state()["radius2"]
    assert (r2 == np.float32(0.06) * np.float32(0.06)).all()
    unclamped = np.stack(passes).max(axis=(0, 3)) < 14.99         # a clamped value can round to just below 15
    assert unclamped.mean() > 0.5 and (ppm[unclamped] > 0).mean() > 0.5
    np.testing.assert_allclose(sppm[unclamped], ppm[unclamped], rtol=1e-5, atol=0)
