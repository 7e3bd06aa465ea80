"""The case table of the path-tracing coverage suite (pt_cases.py) on the CPU oracle and the host tree builder alone:
conditions that keep the GPU comparison of tests/test_gpu_pt_coverage.py from being vacuous, and the CPU form of the
claim k_trace makes about its hardware reciprocal -- the host walk of the exported quantised tree returns the scan's
image when every reciprocal is moved one or two float neighbours either way."""
import numpy as np
import pytest

import guides_oracle
import pt_cases as pc

GEOMETRY = [c.name for c in pc.GEOMETRY]
RAYS = ("closest_rays", "shadow_rays")


@pytest.fixture(scope="module")
def glib(tmp_path_factory):
    return guides_oracle.build(tmp_path_factory.mktemp("guides_oracle"))


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_case_is_not_vacuous(oracle_mod, name):
    case = pc.CASE_BY_NAME[name]
    args, img, st = pc.reference(oracle_mod, name)
    W, H, spp = args[4], args[5], args[7]
    if name in GEOMETRY:
        assert W <= 48 and H <= 40 and spp <= 3
    for a in args[:3]:                                                   # no coordinate the oracle defines nothing for
        for k in ("pos", "center", "v0", "v1", "v2"):
            if a.dtype.names and k in a.dtype.names and len(a):
                assert np.isfinite(a[k]).all() and np.abs(a[k]).max() < 1e18
    assert img.shape == (H, W, 3) and np.isfinite(img).all() and img.min() >= 0.0
    lit = pc.lit_share(img)
    print("%s: lit %.3f, closest rays %d, shadow rays %d" % (name, lit, st["closest_rays"], st["shadow_rays"]))
    assert img.any() and st["closest_rays"] >= st["samples"] == W * H * spp and st["shadow_rays"] > 0
    if case.dark is None:
        assert lit >= 0.5, lit


def test_dark_cases_are_the_named_ones():
    assert {c.name for c in pc.CASES if c.dark} == set(pc.DARK)
    assert all(isinstance(c.dark, str) and len(c.dark) > 10 for c in pc.CASES if c.dark)
    assert len(pc.GEOMETRY) == 15 and set(pc.GUIDES) == set(GEOMETRY) - {"floor-only"}


@pytest.mark.parametrize("name", GEOMETRY)
def test_walk_of_the_exported_tree_equals_the_scan(hpt, oracle_mod, name):
    """Bytes and ray counts; then again with the three reciprocals of every ray moved 1 and 2 ulps in each of the 8
    combinations of directions.  A failure here means the +-1 cell margin of the quantised planes (scene_build.cpp) or
    the 2e-6 slack of the slab test does not cover a reciprocal that is a neighbour of the exact one."""
    args, scan, s_scan = pc.reference(oracle_mod, name)
    bvh = pc.tree(hpt, name)
    walk, s_walk = pc.oracle_render(oracle_mod, args, bvh=bvh)
    assert np.array_equal(walk, scan)
    assert all(s_walk[k] == s_scan[k] for k in RAYS)
    assert s_walk["boxes_closest"] >= 2 * s_walk["closest_rays"] and s_walk["tris_closest"] > 0
    for ulps in (1, 2):
        for mask in range(8):
            img, st = pc.oracle_render(oracle_mod, args, bvh=bvh, rcp_nudge=(ulps, mask))
            assert np.array_equal(img, scan), (ulps, mask)
            assert all(st[k] == s_scan[k] for k in RAYS), (ulps, mask)


def test_the_nudge_reaches_the_walk_and_only_the_walk(hpt, oracle_mod):
    """A large nudge changes the walk's box counts (the option is wired to the reciprocals); without a tree the option
    does nothing at all."""
    args, scan, s_scan = pc.reference(oracle_mod, "far64")
    bvh = pc.tree(hpt, "far64")
    _, exact = pc.oracle_render(oracle_mod, args, bvh=bvh)
    _, zero = pc.oracle_render(oracle_mod, args, bvh=bvh, rcp_nudge=(0, 5))
    _, moved = pc.oracle_render(oracle_mod, args, bvh=bvh, rcp_nudge=(4096, 5))
    assert zero == exact and moved["boxes_closest"] != exact["boxes_closest"]
    img, st = pc.oracle_render(oracle_mod, args, rcp_nudge=(4096, 5))
    assert np.array_equal(img, scan) and st == s_scan


@pytest.mark.parametrize("name", pc.GUIDES)
def test_guides_cover_the_image(glib, oracle_mod, name):
    L, sp, tr, cam, W, H, depth, spp, kw = pc.CASE_BY_NAME[name].make()
    g, hp = guides_oracle.render(glib, L, sp, tr, cam, W, H, 1, seed=kw["seed"])
    cov = float((g["coverage"] > 0).mean())
    print("%s: guide coverage %.3f" % (name, cov))
    assert cov >= 0.5 and hp == [int(g["coverage"].sum())]
    assert all(np.isfinite(g[k]).all() for k in g)


def _differ(a, b):
    return int((a != b).any(axis=-1).sum())


def test_max_delta_takes_effect(oracle_mod):
    default, _ = pc.oracle_render(oracle_mod, pc.max_delta_case(0))
    images = [pc.reference(oracle_mod, "max_delta-%d" % m)[1] for m in pc.MAX_DELTAS] + [default]
    changed = [_differ(img, default) for img in images]
    print("pixels changed by caps 1, 2, 3 against the default: %s" % changed[:3])
    assert changed[0] > changed[1] > changed[2] > 0
    assert all(_differ(images[k], images[k + 1]) > 0 for k in range(3))
    assert np.array_equal(pc.oracle_render(oracle_mod, pc.max_delta_case(8))[0], default)


def test_mirror_box_reaches_the_cap(oracle_mod):
    refs = [pc.reference(oracle_mod, "mirror-%d" % m) for m in pc.MIRROR_DELTAS]
    assert pc.MIRROR_DELTAS[-1] == pc.MAX_DELTA_CAP
    per_sample = [st["delta_bounces"] / st["samples"] for _, _, st in refs]
    print("delta bounces per sample at caps 8, 64, 250: %s" % per_sample)
    assert per_sample[0] > 8 and per_sample[1] > 50 and per_sample[2] > 100
    assert _differ(refs[0][1], refs[1][1]) > 0 and _differ(refs[1][1], refs[2][1]) > 0
    _, s249 = pc.oracle_render(oracle_mod, pc.mirror_box_case(249))
    assert s249["closest_rays"] < refs[2][2]["closest_rays"]              # paths are still alive at the 250th delta bounce
    # the library clamps: the table asks the oracle for 250 where a caller asks for more
    for m in pc.MIRROR_CLAMPED:
        assert m > pc.MAX_DELTA_CAP and pc.oracle_kw(pc.mirror_box_case(m)[8])["max_delta"] == pc.MAX_DELTA_CAP


def test_depth_and_roulette_take_effect(oracle_mod):
    plain = [pc.reference(oracle_mod, "depth-%d" % d) for d in pc.DEPTHS]
    rr = [pc.reference(oracle_mod, "depth-%d-rr" % d) for d in pc.DEPTHS]
    rays = [st["closest_rays"] for _, _, st in plain]
    print("closest rays at depths %s: %s" % (pc.DEPTHS, rays))
    assert all(a < b for a, b in zip(rays, rays[1:]))
    assert all(_differ(plain[k][1], plain[k + 1][1]) > 0 for k in range(len(plain) - 1))
    for d, p, r in zip(pc.DEPTHS, plain, rr):
        if d == 1:
            assert np.array_equal(p[1], r[1])                            # the roulette is played after a bounce: none at depth 1
        else:
            assert _differ(p[1], r[1]) > 0 and r[2]["closest_rays"] < p[2]["closest_rays"]


def test_high_seed_words_and_the_offset_take_effect(oracle_mod):
    images = []
    for k, seed in enumerate(pc.HIGH_SEEDS):
        args, img, _ = pc.reference(oracle_mod, "seed-%d" % k)
        assert args[8]["seed"] == seed and seed >> 32
        low, _ = pc.oracle_render(oracle_mod, pc.seed_case(seed & 0xFFFFFFFF))
        assert _differ(img, low) > 100
        images.append(img)
    assert _differ(images[0], images[1]) > 100 and _differ(images[1], images[2]) > 100
    args, img, _ = pc.reference(oracle_mod, "offset")
    assert args[8]["sample_offset"] == pc.BIG_OFFSET == 2**31 - 8 and args[7] == 4
    for other in (0, pc.BIG_OFFSET - 1, pc.BIG_OFFSET & 0xFFFF):
        assert _differ(img, pc.oracle_render(oracle_mod, pc.seed_case(8, other, 4))[0]) > 100
    args, img, _ = pc.reference(oracle_mod, "wrapper-seed")
    assert args[8]["seed"] == 2**62
    assert _differ(img, pc.oracle_render(oracle_mod, pc.seed_case(0))[0]) > 100


@pytest.mark.parametrize("name", sorted(pc.ZERO_COMPONENT))
def test_zero_component_cameras_give_exact_zeros(name):
    L, sp, tr, cam, W, H = pc.CASE_BY_NAME[name].make()[:6]
    for jitter in (0.0, 0.25, 0.99999994):
        d = pc.primary_dirs(cam, W, H, jitter)
        assert np.isfinite(d).all()
        assert (d[..., 1] == 0).all()
        if pc.ZERO_COMPONENT[name] == "xy":
            assert (d[..., 0] == 0).all() and (d[..., 2] == 1).all()
        else:
            assert (d[..., 0] != 0).mean() > 0.9 and (d[..., 2] > 0).all()
    if name == "camera-floor":
        assert float(cam["eye"][1]) == -0.5 and (tr["v0"][:2, 1] == -0.5).all()


def test_geometry_cases_are_what_they_say(hpt):
    assert pc.tree(hpt, "deep-far")["bvh_depth"] > 12
    far = pc.CASE_BY_NAME["deep-far"].make()
    assert len(far[2]) == 20012 and (far[4], far[5], far[6], far[7]) == (32, 24, 3, 2)
    # the sliver stretches the x grid to cells of 0.076; the other axes keep the box's
    q = pc.tree(hpt, "sliver")["qscale"]
    assert 0.07 < q[0] < 0.08 and q[1] < 1e-4 and q[2] < 1e-4
    flat = pc.tree(hpt, "floor-only")
    assert flat["num_nodes"] == 1 and flat["num_tris"] == 2
    # zero-area triangles and more identical ones than a leaf holds
    tr = pc.CASE_BY_NAME["degenerate"].make()[2]
    v0, v1, v2 = (tr[k].astype(np.float64) for k in ("v0", "v1", "v2"))
    area = np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)
    assert (area == 0).sum() >= 2 and (area < 1e-7).sum() == 3
    assert ((v0 == v1).all(axis=1) & (v1 == v2).all(axis=1)).sum() == 1 and ((v0 == v1).all(axis=1)).sum() == 2
    same = (v0 == v0[-1]).all(axis=1) & (v1 == v1[-1]).all(axis=1) & (v2 == v2[-1]).all(axis=1)
    assert same.sum() == pc.N_IDENTICAL == 9 and same[-9:].all()
    bvh = pc.tree(hpt, "degenerate")
    assert bvh["num_tris"] == len(tr)
    L, sp, tr = pc.CASE_BY_NAME["many-rounds"].make()[:3]
    assert (len(sp), len(L)) == (64, 40) and len({float(e) > 0 for e in sp["mtl"]["eta"]}) == 2
    for name, (s, sh) in (("far64", (64.0, 300.0)), ("shift-16384", (1.0, 16384.0)), ("scale-4096", (4096.0, 0.0)), ("scale-1/64", (1 / 64.0, 0.0))):
        v = pc.CASE_BY_NAME[name].make()[2]["v0"][:, 0]
        assert abs(float(v.max() - v.min()) - s) < 0.01 * s and abs(float(v.min()) - (sh - 0.5 * s)) < 0.01 * s + 1e-3 * abs(sh)


@pytest.mark.parametrize("what,count", pc.STAGING)
def test_staging_cases_sit_on_the_limits(what, count):
    L, sp, tr = pc.CASE_BY_NAME["%s-%d" % (what, count)].make()[:3]
    assert (pc.n_materials(sp, tr) if what == "mats" else len(L)) == count
    assert count in (128, 129, 32, 33)


def test_shape_and_rank_cases():
    assert pc.SHAPES == [(1, 1), (7, 3), (8, 8), (9, 65), (1, 257)] and pc.SHAPE_TILES == [8, 32, 1024]
    assert pc.SHAPE_SPP == [(1, 0), (5, 2)]
    for name, (W, H, tile, worlds) in pc.RANKS.items():
        tiles = -(-W // tile) * -(-H // tile)
        assert any(w > tiles for w in worlds) == (name == "ranks-40x24")
    assert pc.RANKS["ranks-40x24"][2:] == (32, (3, 8)) and pc.RANKS["ranks-50x37"][2:] == (8, (5, 7))
