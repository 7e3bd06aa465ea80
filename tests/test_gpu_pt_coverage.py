"""The unidirectional path tracer on the MI355X against the CPU oracle at the cases of pt_cases.py.

Geometry and camera cases reach k_trace the only way rays reach it -- through render_pt and render_guides: every case
is rendered at the default node-step budget, at a budget of 1 (practically every ray takes the four-wide resume walk)
and unsplit, once more with the counting kernel (whose work counts are the host walk's of the exported tree, ray for
ray), and as first-hit guide buffers at one sample per pixel, where a wrong hit is wrong bytes even in a black pixel.
Parameter cases cover eye depths 1 to 40 with and without roulette, delta caps down to 1 and up to the clamp, images
smaller than a sub-tile and tiles larger than the image, ranks without a pixel, the high words of seed and sample
offset, and the LDS staging limits of k_shade met exactly.

Every comparison is np.array_equal: oracle and kernels evaluate the same IEEE expressions in the same order.
tests/test_pt_cases_cpu.py keeps the oracle images of these cases from being black or indifferent to their parameter."""
import numpy as np
import pytest

import guides_oracle
import pt_cases as pc
from test_bvh_walk import COUNT_KEYS

pytestmark = pytest.mark.gpu

GEOMETRY = [c.name for c in pc.GEOMETRY]
GUIDE_KEYS = ("albedo", "normal", "position", "coverage")
_WALKS = {}


@pytest.fixture(scope="module")
def glib(tmp_path_factory):
    return guides_oracle.build(tmp_path_factory.mktemp("guides_oracle"))


def _walk(hpt, oracle_mod, name):
    """(image, stats) of the oracle walking the exported tree of a geometry case: shared, not to be written to."""
    if name not in _WALKS:
        _WALKS[name] = pc.oracle_render(oracle_mod, pc.reference(oracle_mod, name)[0], bvh=pc.tree(hpt, name))
    return _WALKS[name]


def _params(hpt, kw, budget=0, **more):
    flags = kw.get("flags", 0) | more.get("flags", 0)            # a case's own flag (roulette) stays on
    p = hpt.make_params(**dict(kw, **dict(more, flags=flags)))
    p.reserved = budget << 1
    return p


def _render(hpt, scene, args, budget=0, **more):
    L, sp, tr, cam, W, H, depth, spp, kw = args
    return scene.render_pt(cam, W, H, depth, spp, _params(hpt, kw, budget, **more))


def _report(what, img, ref):
    print("%s: %d of %d pixels differ, max abs %.3e" % (what, int((img != ref).any(axis=-1).sum()), ref.shape[0] * ref.shape[1],
                                                        float(np.abs(img - ref).max())))


@pytest.mark.parametrize("name", GEOMETRY)
def test_geometry_case_matches_the_oracle(hpt, oracle_mod, name):
    args, ref, ref_st = pc.reference(oracle_mod, name)
    host_tree = pc.tree(hpt, name)
    walk, walk_st = _walk(hpt, oracle_mod, name)
    assert np.array_equal(walk, ref)
    with hpt.Scene(*args[:3]) as scene:
        dev_tree = scene.export_bvh()
        images, resumes = {}, {}
        for budget in (0, 1, 63):                      # default (6), practically every ray resumes, unsplit
            images["budget %d" % budget] = _render(hpt, scene, args, budget)
            images["budget %d, timed" % budget] = _render(hpt, scene, args, budget, flags=hpt.FLAG_TIME_KERNELS)
            resumes[budget] = scene.stats()["n_resume"]
        images["counted"] = _render(hpt, scene, args, flags=hpt.FLAG_COUNT_WORK)
        st = scene.stats()
    for k in ("qnodes", "tris", "qorigin", "qscale"):
        assert np.array_equal(dev_tree[k], host_tree[k]), k
    for what, img in images.items():
        _report(what, img, ref)
    got = {k: int(st[k]) for k in COUNT_KEYS}
    want = {k: int(walk_st[k]) for k in COUNT_KEYS}
    print("work counts: device %s, host walk %s; resume launches %s" % (got, want, resumes))
    for what, img in images.items():
        assert np.array_equal(img, ref), what
    assert got == want
    assert want["closest_rays"] == ref_st["closest_rays"] and want["shadow_rays"] == ref_st["shadow_rays"]
    assert resumes[0] > 0 and resumes[1] > 0 and resumes[63] == 0
    if name == "deep-far":
        assert st["bvh_depth"] > 12


@pytest.mark.parametrize("name", GEOMETRY)
def test_geometry_case_first_hits_match_the_oracle(hpt, glib, name):
    """render_guides at one sample per pixel: the first non-delta hit of one ray per pixel, found by the first trace
    launch plus its resume launch at the default budget."""
    L, sp, tr, cam, W, H, depth, spp, kw = pc.CASE_BY_NAME[name].make()
    with hpt.Scene(L, sp, tr) as scene:
        got = scene.render_guides(cam, W, H, 1, hpt.make_params(seed=kw["seed"]))
        hits = scene.ppm_stats()["hit_points"]
    ref, hp = guides_oracle.render(glib, L, sp, tr, cam, W, H, 1, seed=kw["seed"])
    for k in GUIDE_KEYS:
        print("%s: %d values differ" % (k, int((got[k] != ref[k]).sum())))
    assert hits == sum(hp) > 0
    for k in GUIDE_KEYS:
        assert got[k].tobytes() == ref[k].tobytes(), k


@pytest.mark.parametrize("roulette", [False, True])
def test_flag_matrix_far_from_the_origin(hpt, oracle_mod, roulette):
    args = list(pc.reference(oracle_mod, "far64")[0])
    rr = hpt.FLAG_RUSSIAN_ROULETTE if roulette else 0
    assert rr == (pc.FLAG_RUSSIAN_ROULETTE if roulette else 0)
    args[8] = dict(args[8], flags=rr)
    ref, ref_st = pc.oracle_render(oracle_mod, tuple(args))
    other, _ = pc.oracle_render(oracle_mod, tuple(args[:8]) + (dict(args[8], flags=rr ^ pc.FLAG_RUSSIAN_ROULETTE),))
    assert not np.array_equal(ref, other)
    with hpt.Scene(*args[:3]) as scene:
        for flags in (hpt.FLAG_COUNT_WORK, hpt.FLAG_BRUTE_FORCE, hpt.FLAG_SINGLE_PIPELINE, 0):
            img = _render(hpt, scene, args, flags=rr | flags)
            _report("flags %d" % (rr | flags), img, ref)
            assert np.array_equal(img, ref), flags
            if flags == hpt.FLAG_COUNT_WORK:
                st = scene.stats()
                assert st["closest_rays"] == ref_st["closest_rays"] and st["shadow_rays"] == ref_st["shadow_rays"]


PLAIN = ([c.name for c in pc.PARAMETERS if c.name.split("-")[0] in ("depth", "max_delta", "mirror", "seed", "offset", "mats", "lights")])


@pytest.mark.parametrize("name", PLAIN)
def test_parameter_case_matches_the_oracle(hpt, oracle_mod, name):
    """The default render path and the counting one: the oracle's bytes and the oracle's rays."""
    args, ref, ref_st = pc.reference(oracle_mod, name)
    with hpt.Scene(*args[:3]) as scene:
        n_mats = scene.stats()["n_materials"]
        img = _render(hpt, scene, args)
        counted = _render(hpt, scene, args, flags=hpt.FLAG_COUNT_WORK)
        st = scene.stats()
        low = None
        if name.startswith("seed-"):
            low = _render(hpt, scene, args[:8] + (dict(args[8], seed=args[8]["seed"] & 0xFFFFFFFF),))
    _report(name, img, ref)
    print("rays: device %d + %d, oracle %d + %d" % (st["closest_rays"], st["shadow_rays"], ref_st["closest_rays"], ref_st["shadow_rays"]))
    assert np.array_equal(img, ref) and np.array_equal(counted, ref)
    assert st["closest_rays"] == ref_st["closest_rays"] and st["shadow_rays"] == ref_st["shadow_rays"]
    if low is not None:
        assert not np.array_equal(low, ref)                         # the high word of hpt_params.seed reaches the streams
    what, _, count = name.partition("-")
    if what == "mats":
        assert n_mats == int(count) and len(args[0]) <= 32
    if what == "lights":
        assert len(args[0]) == int(count) and n_mats <= 128


def _device_render(hpt, scene, args, params):
    """render_pt_device + untile of a whole image on the current stream: (image, packed local buffer)."""
    import torch
    L, sp, tr, cam, W, H, depth, spp, kw = args
    stream = torch.cuda.current_stream().cuda_stream
    n_local = hpt.local_pixels(W, H, hpt.make_params())
    local = torch.full((n_local, 3), 7.0, dtype=torch.float32, device="cuda")
    scene.render_pt_device(cam, W, H, depth, spp, params, local.data_ptr(), stream)
    image = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    hpt.untile(local.data_ptr(), image.data_ptr(), W, H, hpt.make_params(), stream)
    torch.cuda.synchronize()
    return image.cpu().numpy(), local.cpu().numpy()


def test_delta_cap_is_clamped_and_reached_blind(hpt, oracle_mod):
    """max_delta above 250 renders 250's image (take_params clamps), and the 250 case with HPT_FLAG_NO_HOST_WAIT enqueues
    its 254 iterations unseen and still ends every path where the oracle does."""
    args, ref, _ = pc.reference(oracle_mod, "mirror-250")
    with hpt.Scene(*args[:3]) as scene:
        for m in pc.MIRROR_CLAMPED:
            clamped = pc.mirror_box_case(m)
            assert clamped[8]["max_delta"] == m
            img = _render(hpt, scene, clamped)
            _report("max_delta %d" % m, img, ref)
            assert np.array_equal(img, ref), m
        for flags in (0, hpt.FLAG_NO_HOST_WAIT):
            img, _ = _device_render(hpt, scene, args, _params(hpt, args[8], flags=flags))
            _report("device render, flags %d" % flags, img, ref)
            assert np.array_equal(img, ref), flags


@pytest.mark.parametrize("W,H", pc.SHAPES)
def test_small_images_and_large_tiles(hpt, oracle_mod, W, H):
    """Images of less than one 8 x 8 sub-tile up to a few tiles, in tiles of 8, 32 and 1024 (larger than the image), at one
    sample and at five in passes of two (two pipelines, then a one-sample pass on one)."""
    for spp, spass in pc.SHAPE_SPP:
        args, ref, _ = pc.reference(oracle_mod, "shape-%dx%d-spp%d" % (W, H, spp))
        assert args[8].get("samples_per_pass", 0) == spass and ref.any()
        with hpt.Scene(*args[:3]) as scene:
            for tile in pc.SHAPE_TILES:
                img = _render(hpt, scene, args, tile=tile)
                _report("%d spp, tile %d" % (spp, tile), img, ref)
                assert np.array_equal(img, ref), (spp, tile)


@pytest.mark.parametrize("name", sorted(pc.RANKS))
def test_ranks_without_a_pixel(hpt, oracle_mod, name):
    """More ranks than tiles (40 x 24 in two tiles of 32 for 3 and 8 ranks) and rank counts that do not divide the tiles:
    the assembled image is the single-device one and the oracle's; a rank without a tile writes zeros."""
    import torch
    args, ref, _ = pc.reference(oracle_mod, name)
    L, sp, tr, cam, W, H, depth, spp, kw = args
    _, _, tile, worlds = pc.RANKS[name]
    ntiles = -(-W // tile) * -(-H // tile)
    stream = torch.cuda.current_stream().cuda_stream
    with hpt.Scene(L, sp, tr) as scene:
        single = _render(hpt, scene, args, tile=tile)
        assert np.array_equal(single, ref)
        for world in worlds:
            n_local = hpt.local_pixels(W, H, hpt.make_params(world=world, tile=tile))
            gathered = torch.full((world, n_local, 3), 7.0, dtype=torch.float32, device="cuda")
            for r in range(world):
                scene.render_pt_device(cam, W, H, depth, spp, _params(hpt, kw, rank=r, world=world, tile=tile), gathered[r].data_ptr(), stream)
            image = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            hpt.untile(gathered.data_ptr(), image.data_ptr(), W, H, hpt.make_params(world=world, tile=tile), stream)
            torch.cuda.synchronize()
            img, parts = image.cpu().numpy(), gathered.cpu().numpy()
            _report("world %d" % world, img, ref)
            assert np.array_equal(img, single), world
            idle = [r for r in range(world) if r >= ntiles]
            assert bool(idle) == (world > ntiles)
            assert not (parts == 7.0).any()                          # every slot of every rank is written
            for r in idle:
                assert not parts[r].any(), (world, r)
    assert any(w > ntiles for w in worlds) == (name == "ranks-40x24")


def test_one_shot_wrapper_with_a_seed_of_2_to_the_62(hpt, oracle_mod):
    args, ref, _ = pc.reference(oracle_mod, "wrapper-seed")
    L, sp, tr, cam, W, H, depth, spp, kw = args
    hpt.wrapper_cache_clear()
    img = hpt.pt_render_wrapper(L, sp, tr, cam, W, H, depth, spp, seed=kw["seed"])
    hpt.wrapper_cache_clear()
    _report("wrapper", img, ref)
    assert kw["seed"] == 2**62 and np.array_equal(img, ref)


def test_workspace_reuse_across_image_sizes(hpt, oracle_mod):
    """One scene renders 1 x 1, 48 x 40, 7 x 3 and 48 x 40 again: the workspace grows once and is reused for smaller and
    equal shapes; the two 48 x 40 images are the same and the oracle's."""
    images = []
    with hpt.Scene(*pc._input(1, 1)[:3]) as scene:
        for W, H in ((1, 1), (48, 40), (7, 3), (48, 40)):
            args = pc.shape_case(W, H, 2, 0)
            images.append((args, _render(hpt, scene, args)))
    for args, img in images:
        ref, _ = pc.oracle_render(oracle_mod, args)
        _report("%d x %d" % (args[4], args[5]), img, ref)
        assert np.array_equal(img, ref)
    assert np.array_equal(images[1][1], images[3][1]) and images[1][1].mean() > 0.01
