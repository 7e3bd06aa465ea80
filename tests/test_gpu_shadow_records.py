"""Shadow-ray records indexed by queue position (csrc: flush_nee in k_shade, pt_shade.hip; the any-hit side of
trace_chunk, pt_trace.hip; k_connect, pt_scan.hip) against the CPU oracle and against renders whose records land somewhere else.

k_shade stores the record of a next-event candidate at `first queue position of the workgroup's chunk + rank among the
chunk's records`, the shadow queue lists those indices, and the path slot rides in contrib.w.  Where a record lands
therefore depends on the chunk size (256 to 1024 entries, from the queue length), on the samples per pass, on the number
of pipelines and on whether the grid walks its chunks with a stride; the image must depend on none of them.  Every case
is rendered at least twice with records in different places (one pass against passes of one sample, the trace kernels
against k_connect of HPT_FLAG_BRUTE_FORCE, one pipeline against two) and compared with np.array_equal, among the renders
and with oracle.pt_render (a window of it where the whole image would take the oracle long).

  chunk shapes     cornell_diffuse (36 triangles) at 512 x 512 x 4 spp: 1 Mi queue entries in one pass (1024-entry chunks,
                   four trips and several flushes per wave), passes of one sample (256-entry chunks), one pipeline, k_connect
  ragged ends      33 x 17 at 3 spp: slots outside the image, a last chunk that is no multiple of 256, short tail queues
  record density   no light (no record at all), a light shut into a box (every shadow ray blocked: a black image), the floor
                   alone under a parallel light (every hit leaves a record, none is blocked), a ball light and a parallel
                   one in one open scene (both branches of flush_nee in one wave)
  deferred rays    cornell_with_sphere(2000) at 64 x 64 x 4 spp with the default node-step budget (shadow rays reach the resume
                   launch as record indices through s_long) and unsplit
  strided launches a mirror box with a diffuse floor at 1024 x 1024 x 6 spp, eye depth 1, max_delta 4, HPT_FLAG_NO_HOST_WAIT:
                   the tail iterations run on a grid of 8 workgroups per CU (2048 on the MI355X) and their queues hold more
                   than 2048 chunks of 1024 entries, so a workgroup shades several chunks with a `begin` of its own each
  two ranks        50 x 37 in 35 tiles of 8 over ranks 0 and 1: the local slot count is not W x H, and rank 1 owns a tile less
"""
import numpy as np
import pytest

import pt_cases as pc
from path_tracing_amd import scene_io as sio
from path_tracing_amd.layouts import LIGHT

pytestmark = pytest.mark.gpu

NO_SPLIT = 63                       # hpt_params.reserved budget bits: the trace step is not split


def _params(hpt, kw, budget=0, **more):
    p = hpt.make_params(**dict(kw, **more))
    p.reserved = budget << 1
    return p


def _render(hpt, scene, args, budget=0, **more):
    L, sp, tr, cam, W, H, depth, spp, kw = args
    return scene.render_pt(cam, W, H, depth, spp, _params(hpt, kw, budget, **more))


def _check(images, ref, window=None):
    """Every image is the first one; the first one is the oracle's inside `window` = (x0, y0, x1, y1)."""
    x0, y0, x1, y1 = window if window else (0, 0, ref.shape[1], ref.shape[0])
    names = list(images)
    first = images[names[0]]
    for what in names:
        img = images[what]
        print("%s: %d pixels differ from '%s', %d of the window's from the oracle (max abs %.3e), mean %.5f" % (
            what, int((img != first).any(axis=-1).sum()), names[0], int((img[y0:y1, x0:x1] != ref[y0:y1, x0:x1]).any(axis=-1).sum()),
            float(np.abs(img[y0:y1, x0:x1] - ref[y0:y1, x0:x1]).max()), float(img.mean())))
    assert np.isfinite(first).all()
    assert np.array_equal(first[y0:y1, x0:x1], ref[y0:y1, x0:x1])
    for what in names[1:]:
        assert np.array_equal(images[what], first), what


def _layouts(hpt, scene, args, spp_per_pass=1):
    """The same render with its shadow records in four different places."""
    return {"one pass": _render(hpt, scene, args),
            "passes of %d" % spp_per_pass: _render(hpt, scene, args, samples_per_pass=spp_per_pass),
            "one pipeline": _render(hpt, scene, args, samples_per_pass=spp_per_pass, flags=hpt.FLAG_SINGLE_PIPELINE),
            "k_connect": _render(hpt, scene, args, flags=hpt.FLAG_BRUTE_FORCE)}


def _cornell(W, H, spp, depth=4, seed=11):
    L, sp, tr = sio.cornell_diffuse()
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)
    return L, sp, tr, cam, W, H, depth, spp, dict(seed=seed, samples_per_pass=spp)


# ---- chunk shapes -------------------------------------------------------------------------------------------------------
CHUNK_WINDOW = (224, 300, 288, 364)           # 64 x 64 over the two small boxes and their shadows on the floor


def test_chunk_shapes(hpt, oracle_mod):
    args = _cornell(512, 512, 4)
    assert len(args[2]) == 36 and 512 * 512 * 4 > 786 * 1024          # k_shade's chunk is 1024 entries above 786 Ki
    ref, st = pc.oracle_render(oracle_mod, args, window=CHUNK_WINDOW)
    assert st["shadow_rays"] > 0 and ref.any()
    with hpt.Scene(*args[:3]) as scene:
        images = _layouts(hpt, scene, args)
    _check(images, ref, CHUNK_WINDOW)


# ---- ragged ends --------------------------------------------------------------------------------------------------------
def test_ragged_ends(hpt, oracle_mod):
    args = _cornell(33, 17, 3, seed=4)
    ref, st = pc.oracle_render(oracle_mod, args)
    assert st["shadow_rays"] > 0 and (33 * 17 * 3) % 256 != 0
    with hpt.Scene(*args[:3]) as scene:
        images = _layouts(hpt, scene, args)
        images["counted"] = _render(hpt, scene, args, flags=hpt.FLAG_COUNT_WORK)
        counted = scene.stats()
    _check(images, ref)
    assert counted["shadow_rays"] == st["shadow_rays"] and counted["closest_rays"] == st["closest_rays"]


# ---- extremes of record density -----------------------------------------------------------------------------------------
def _open_box():
    """cornell_diffuse without its ceiling."""
    L, sp, tr = sio.cornell_diffuse()
    up = (tr["v0"][:, 1] == 0.5) & (tr["v1"][:, 1] == 0.5) & (tr["v2"][:, 1] == 0.5)
    assert up.sum() == 2
    tr = tr[~up].copy()
    tr["id"] = np.arange(len(tr))
    return L, sp, tr


def density_case(which):
    W, H, spp = 96, 80, 3
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)
    sun = sio._one_light((0.0, 0.45, 0.3), (0.1, -1.0, 0.2), (0.6, 0.6, 0.6), 0.0, 1, 0.02)
    if which == "no-light":
        _, sp, tr = sio.cornell_diffuse()
        L = np.zeros(0, LIGHT)
    elif which == "all-blocked":
        # the light ball inside the first small box (centre (0.05, 0.1), half width 0.085, y from -0.5 to -0.4)
        _, sp, tr = sio.cornell_diffuse()
        L = sio._one_light((0.05, -0.45, 0.1), (0.0, -1.0, 0.0), (1.0, 1.0, 1.0), 180.0, 0, 0.03)
    elif which == "every-hit":
        # the two floor triangles under a parallel light, seen from 0.8 above: every camera ray meets the floor, a hit
        # always faces the light, nothing is in the way, and the bounce leaves into the sky
        _, sp, tr = sio.cornell_diffuse()
        tr = tr[:2].copy()
        assert (tr["v0"][:, 1] == -0.5).all() and (tr["v1"][:, 1] == -0.5).all() and (tr["v2"][:, 1] == -0.5).all()
        L = sun
        cam = sio.make_camera((0.0, 0.3, 0.0), (0.0, -0.5, 0.0), (0.0, 0.0, 1.0), 50.0, W, H)
    elif which == "ball-and-parallel":
        L, sp, tr = _open_box()
        L = np.concatenate([L, sun])
    else:
        raise KeyError(which)
    return L, sp, tr, cam, W, H, 4, spp, dict(seed=21, samples_per_pass=spp)


DENSITY = ["no-light", "all-blocked", "every-hit", "ball-and-parallel"]
_DENSITY_REF = {}


def density_reference(oracle_mod, which):
    if which not in _DENSITY_REF:
        args = density_case(which)
        img, st = pc.oracle_render(oracle_mod, args)
        img.setflags(write=False)
        _DENSITY_REF[which] = (args, img, st)
    return _DENSITY_REF[which]


@pytest.mark.parametrize("which", DENSITY)
def test_record_density(hpt, oracle_mod, which):
    args, ref, st = density_reference(oracle_mod, which)
    print("oracle: %d closest-hit rays, %d shadow rays, %.1f %% of the pixels lit" % (st["closest_rays"], st["shadow_rays"], 100.0 * pc.lit_share(ref)))
    if which == "no-light":
        assert st["shadow_rays"] == 0 and not ref.any()
    elif which == "all-blocked":
        assert st["shadow_rays"] > 1000 and not ref.any()
    elif which == "every-hit":
        # one shadow ray per camera ray
        assert st["shadow_rays"] >= 0.95 * args[4] * args[5] * args[7] and pc.lit_share(ref) > 0.95
    else:
        assert pc.lit_share(ref) > 0.8
    with hpt.Scene(*args[:3]) as scene:
        images = _layouts(hpt, scene, args)
        images["counted"] = _render(hpt, scene, args, flags=hpt.FLAG_COUNT_WORK)
        counted = scene.stats()
    _check(images, ref)
    assert counted["shadow_rays"] == st["shadow_rays"] and counted["closest_rays"] == st["closest_rays"]


# ---- deferred shadow rays -----------------------------------------------------------------------------------------------
def test_deferred_shadow_rays(hpt, oracle_mod):
    L, sp, tr = sio.cornell_with_sphere(2000)
    W = H = 64
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)
    args = (L, sp, tr, cam, W, H, 4, 4, dict(seed=3, samples_per_pass=4))
    ref, st = pc.oracle_render(oracle_mod, args)
    assert st["shadow_rays"] > 0
    images, resumes = {}, {}
    with hpt.Scene(L, sp, tr) as scene:
        for what, budget in (("default budget", 0), ("budget 1", 1), ("unsplit", NO_SPLIT)):
            images[what] = _render(hpt, scene, args, budget)
            images[what + ", timed"] = _render(hpt, scene, args, budget, flags=hpt.FLAG_TIME_KERNELS)
            resumes[what] = scene.stats()["n_resume"]          # launches are counted by the kernel timers only
        images["passes of 1"] = _render(hpt, scene, args, samples_per_pass=1)
    print("resume launches:", resumes)
    _check(images, ref)
    assert resumes["default budget"] > 0 and resumes["budget 1"] > 0 and resumes["unsplit"] == 0


# ---- strided tail launches ----------------------------------------------------------------------------------------------
STRIDED_W = STRIDED_H = 1024
STRIDED_SPP = 6
STRIDED_WINDOW = (480, 600, 544, 664)         # 64 x 64 of floor in front of the back mirror, the small boxes in it
BLIND_GROUPS, MAX_CHUNK = 8 * 256, 1024       # render_pt.cpp: 8 workgroups per CU (256 on the MI355X); kShadeChunk


def strided_case():
    """cornell_diffuse with every wall but the floor a perfect mirror, eye depth 1: a path is alive past iteration 0 exactly
    while it has met nothing but mirrors, and leaves a shadow record where it ends on the floor or a small box."""
    L, sp, tr = sio.cornell_diffuse()
    tr = tr.copy()
    tr["mtl"]["base_color"][2:12] = 1.0
    tr["mtl"]["roughness"][2:12] = 0.0
    tr["mtl"]["metallic"][2:12] = 1.0
    tr["mtl"]["type"][2:12] = 2
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, STRIDED_W, STRIDED_H)
    return L, sp, tr, cam, STRIDED_W, STRIDED_H, 1, STRIDED_SPP, dict(seed=9, max_delta=4, samples_per_pass=STRIDED_SPP)


def test_strided_tail_launches(hpt, oracle_mod):
    args = strided_case()
    L, sp, tr, cam, W, H, depth, spp, kw = args
    # share of the primary rays whose first hit is a mirror (64 x 64 sample of the image plane): they are the queue of
    # the first tail iteration, which has to hold more chunks than the capped grid has workgroups
    small = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, 64, 64)
    dirs = pc.primary_dirs(small, 64, 64).reshape(-1, 3)
    org = np.tile(np.asarray(small["eye"], np.float32).reshape(1, 3), (len(dirs), 1))
    t, prim = oracle_mod.closest_hits(L, sp, tr, org, dirs)[:2]
    tri = np.asarray(prim) - (len(sp) + len(L))          # the oracle numbers spheres, then light balls, then triangles
    mirror = float(((tri >= 2) & (tri < 12)).mean())
    alive = mirror * W * H * spp
    print("primary rays that meet a mirror: %.1f %%: about %.0f queue entries in the first tail iteration, %d fill the capped grid"
          % (100.0 * mirror, alive, BLIND_GROUPS * MAX_CHUNK))
    assert alive > 1.25 * BLIND_GROUPS * MAX_CHUNK
    ref, st = pc.oracle_render(oracle_mod, args, window=STRIDED_WINDOW)
    assert st["shadow_rays"] > 0 and ref.any()
    with hpt.Scene(L, sp, tr) as scene:
        images = {"host looks": _render(hpt, scene, args),
                  "blind tail": _render(hpt, scene, args, flags=hpt.FLAG_NO_HOST_WAIT),
                  "blind tail, one pipeline, passes of 3": _render(hpt, scene, args, samples_per_pass=3,
                                                                   flags=hpt.FLAG_NO_HOST_WAIT | hpt.FLAG_SINGLE_PIPELINE)}
    _check(images, ref, STRIDED_WINDOW)


# ---- two ranks' tiles ---------------------------------------------------------------------------------------------------
def test_two_ranks(hpt, oracle_mod):
    import torch
    W, H, tile, world, spp = 50, 37, 8, 2, 3
    L, sp, tr = sio.cornell_diffuse()
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)
    kw = dict(seed=15, samples_per_pass=spp)
    args = (L, sp, tr, cam, W, H, 4, spp, kw)
    ref, st = pc.oracle_render(oracle_mod, args)
    assert st["shadow_rays"] > 0
    stream = torch.cuda.current_stream().cuda_stream
    n_local = hpt.local_pixels(W, H, hpt.make_params(world=world, tile=tile))
    assert n_local != W * H and (-(-W // tile) * -(-H // tile)) % world == 1          # rank 0 owns one tile more
    images = {}
    with hpt.Scene(L, sp, tr) as scene:
        images["one device"] = _render(hpt, scene, args, tile=tile)
        for what, more in (("two ranks", {}), ("two ranks, passes of 1", dict(samples_per_pass=1)), ("two ranks, k_connect", dict(flags=hpt.FLAG_BRUTE_FORCE))):
            gathered = torch.full((world, n_local, 3), 7.0, dtype=torch.float32, device="cuda")
            for r in range(world):
                scene.render_pt_device(cam, W, H, 4, spp, _params(hpt, kw, rank=r, world=world, tile=tile, **more), gathered[r].data_ptr(), stream)
            image = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            hpt.untile(gathered.data_ptr(), image.data_ptr(), W, H, hpt.make_params(world=world, tile=tile), stream)
            torch.cuda.synchronize()
            images[what] = image.cpu().numpy()
            assert not (gathered.cpu().numpy() == 7.0).any()
    _check(images, ref)
