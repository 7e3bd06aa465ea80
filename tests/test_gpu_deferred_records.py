"""Closest-hit rays set aside as dense records (csrc/pt_trace.hip: the `defer` block and the resume refill of trace_chunk,
k_trace's hand-off to lqueue[0]) against the CPU oracle and against renders whose records land somewhere else.

Past iteration 0 the first trace launch writes a ray it sets aside as a record of three 16-byte cells ({origin, best t},
{direction, path slot}, {best primitive, its ordinal}) at `first queue position of the workgroup's chunk + rank among the
chunk's deferred rays`; lqueue[0] lists those indices and the resume launch starts the ray from the record alone, writing pb.hit[slot] at
the end.  Where a record lands depends on the chunk size (256 rays below 1 Mi queue entries, 2048 from there), on the
node-step budget (how many rays of a chunk are set aside), on the samples per pass, the number of pipelines and on
whether the grid walks its chunks with a stride; the image must depend on none of them.  The budget is set through
hpt_params.reserved = budget << 1 (63: the step is not split).  Every case is rendered with its records in different
places and compared with np.array_equal, among the renders and with oracle.pt_render (a window of it where the whole
image would take the oracle long).

  short chunks     cornell_with_sphere(2000) at 64 x 64 x 4 spp, depth 4: default budget, budgets 1, 2 and 3 (nearly every ray
                   that meets the tree is set aside, so a chunk's range fills), unsplit; one pass, passes of one sample, one pipeline
  2048-ray chunks  the same scene at 512 x 512 x 4 spp (1 Mi primary rays), default budget and budget 1 against unsplit, the
                   oracle on a 64 x 64 window over the sphere's silhouette.  1.4 % of the primary rays end on the light ball, so
                   iteration 1 falls just under 1 Mi entries and back to 256-ray chunks: the same renders at 5 spp keep iteration 1
                   above 1 Mi, where at budget 1 a chunk's records run up against the next chunk's first place
  ragged           33 x 17 x 3 spp: slots outside the image, a last chunk that is no multiple of 256
  sphere hit       pt_cases.many_rounds_case() with a 112-triangle ball added, budgets 1 and 2: the partial hit of a ray that
                   is set aside is a sphere or a light ball, and best_prim carries the round flag through the record
  ties             coincident triangles of different materials, the ordinal decides the image: two copies (they share a leaf
                   one node step below the root) and ten (more than a leaf holds: the builder cuts them into six leaves three
                   and four steps down), beside 300 small triangles in a corner.  At budget 3 a ray reaches one of the shallow
                   leaves, is set aside with that copy as its partial hit and meets the other copies, at the same t, in the
                   resume launch: the record's ordinal decides whether they replace it
  iteration 0      eye depth 1 (PRIMARY launches and the shadow tail only) and eye depth 2: lqueue[0] holds path slots in
                   iteration 0 and record indices in the next
  strided launches cornell_with_sphere(2000) with every wall but the floor a mirror, 1024 x 1024 x 6 spp, eye depth 1, max_delta 4,
                   with and without HPT_FLAG_NO_HOST_WAIT: iteration 1 holds about 4.5 Mi rays = 2240 chunks of 2048 on a grid
                   capped at 2048 workgroups, so a workgroup walks two chunks, each with a `begin` of its own
  two ranks        50 x 37 in 35 tiles of 8 over ranks 0 and 1
  workspace growth one Scene renders 64 x 64, 256 x 256 and 64 x 64 again: the record arrays are reallocated with the others
"""
import numpy as np
import pytest

import pt_cases as pc
from path_tracing_amd import scene_io as sio

pytestmark = pytest.mark.gpu

NO_SPLIT = 63                       # hpt_params.reserved budget bits: the trace step is not split
N_WALLS = 12                        # cornell_with_sphere: floor (2 triangles), left, right, back, front, ceiling, then the ball


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


def _cam(W, H):
    return sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, W, H)


def _ball_box(W, H, spp, depth=4, seed=3, **kw):
    L, sp, tr = sio.cornell_with_sphere(2000)
    return L, sp, tr, _cam(W, H), W, H, depth, spp, dict(dict(seed=seed, samples_per_pass=spp), **kw)


def _long_share(scene):
    st = scene.stats()
    return st["long_rays_last_pass"] / max(st["traced_rays_last_pass"], 1)


# ---- short chunks -------------------------------------------------------------------------------------------------------
def test_short_chunks(hpt, oracle_mod):
    args = _ball_box(64, 64, 4)
    ref, st = pc.oracle_render(oracle_mod, args)
    assert st["closest_rays"] > 64 * 64 * 4 and ref.any()
    images, share = {}, {}
    with hpt.Scene(*args[:3]) as scene:
        for what, budget in (("default budget", 0), ("budget 1", 1), ("budget 2", 2), ("budget 3", 3), ("unsplit", NO_SPLIT)):
            images[what] = _render(hpt, scene, args, budget)
            share[what] = _long_share(scene)
            if budget != NO_SPLIT:
                images[what + ", passes of 1"] = _render(hpt, scene, args, budget, samples_per_pass=1)
                images[what + ", one pipeline"] = _render(hpt, scene, args, budget, samples_per_pass=1, flags=hpt.FLAG_SINGLE_PIPELINE)
    print("rays set aside, share of the last pass's:", share)
    _check(images, ref)
    # a ray that enters the box of the tree's root takes more than three node steps
    assert share["budget 1"] > 0.5 and share["budget 3"] > 0.5 and 0.0 < share["default budget"] < share["budget 3"] and share["unsplit"] == 0.0


# ---- 2048-ray chunks ----------------------------------------------------------------------------------------------------
BIG_WINDOW = (344, 150, 408, 214)             # 64 x 64 over the right edge of the ball (columns 248 to 376, rows 112 to 240)


@pytest.mark.parametrize("spp", [4, 5])
def test_long_chunks(hpt, oracle_mod, spp):
    args = _ball_box(512, 512, spp)
    L, sp, tr, cam, W, H = args[:6]
    assert W * H * 4 >= 1 << 20                                       # kTraceShortQueue: chunks of 2048 rays from here
    # the primary rays that start no second ray: they end on the light ball (64 x 64 sample of the image plane)
    small = _cam(64, 64)
    dirs = pc.primary_dirs(small, 64, 64).reshape(-1, 3)
    org = np.tile(np.asarray(small["eye"], np.float32).reshape(1, 3), (len(dirs), 1))
    prim = np.asarray(oracle_mod.closest_hits(L, sp, tr, org, dirs)[1])
    ended = float((prim < len(sp) + len(L)).mean())
    second = (1.0 - ended) * W * H * spp
    print("%.1f %% of the primary rays end on the light: about %.0f rays in iteration 1 (1 Mi = %d)" % (100.0 * ended, second, 1 << 20))
    if spp == 5:
        assert second > 1.1 * (1 << 20)
    ref, st = pc.oracle_render(oracle_mod, args, window=BIG_WINDOW)
    x0, y0, x1, y1 = BIG_WINDOW
    assert 0.2 < pc.lit_share(ref[y0:y1, x0:x1]) and st["closest_rays"] > 64 * 64 * spp
    with hpt.Scene(L, sp, tr) as scene:
        images = {"unsplit": _render(hpt, scene, args, NO_SPLIT),
                  "default budget": _render(hpt, scene, args),
                  "budget 1": _render(hpt, scene, args, 1)}
        share = _long_share(scene)
    print("budget 1: %.1f %% of the last pass's rays set aside" % (100.0 * share))
    assert share > 0.5
    _check(images, ref, BIG_WINDOW)


# ---- ragged -------------------------------------------------------------------------------------------------------------
def test_ragged(hpt, oracle_mod):
    args = _ball_box(33, 17, 3, seed=4)
    ref, st = pc.oracle_render(oracle_mod, args)
    assert (33 * 17 * 3) % 256 != 0 and ref.any()
    with hpt.Scene(*args[:3]) as scene:
        images = {"unsplit": _render(hpt, scene, args, NO_SPLIT)}
        for budget in (0, 1, 3):
            images["budget %d" % budget] = _render(hpt, scene, args, budget)
            images["budget %d, passes of 1" % budget] = _render(hpt, scene, args, budget, samples_per_pass=1)
            images["budget %d, tiles of 8" % budget] = _render(hpt, scene, args, budget, tile=8)
    _check(images, ref)


# ---- the partial hit is a sphere ----------------------------------------------------------------------------------------
def test_partial_hit_is_a_sphere(hpt, oracle_mod):
    L, sp, tr, cam, W, H, depth, spp, kw = pc.many_rounds_case()
    ball = sio._tris_from(sio.tessellated_sphere((0.1, -0.25, 0.5), 0.12, 8, 8), [(0.8, 0.6, 0.2, 1.0, 0.0, 0.0)] * 112)
    tr = np.concatenate([tr, ball])
    tr["id"] = np.arange(len(tr))
    args = (L, sp, tr, cam, W, H, depth, spp, dict(kw, samples_per_pass=spp))
    ref, st = pc.oracle_render(oracle_mod, args)
    assert len(sp) == pc.N_SPHERES and pc.lit_share(ref) > 0.5
    images, share = {}, {}
    with hpt.Scene(L, sp, tr) as scene:
        for what, budget in (("unsplit", NO_SPLIT), ("budget 1", 1), ("budget 2", 2), ("default budget", 0)):
            images[what] = _render(hpt, scene, args, budget)
            share[what] = _long_share(scene)
        images["budget 1, passes of 1"] = _render(hpt, scene, args, 1, samples_per_pass=1)
    print("rays set aside, share of the last pass's:", share)
    # at budget 1 every ray that meets the root's box is set aside, those whose nearest sphere is in front of the walls too
    assert share["budget 1"] > 0.5
    _check(images, ref)


# ---- ties ---------------------------------------------------------------------------------------------------------------
def ties_case(copies):
    """`copies` identical triangles across the view (the materials alternate between two hues and grow greener), between
    two halves of 300 small triangles in the lower right far corner; no walls, so the copies hang a few node steps below the root."""
    L, sp, _ = sio.cornell_diffuse()
    rng = np.random.default_rng(5)
    n = 300
    c = rng.uniform([0.2, -0.45, 0.6], [0.45, -0.2, 0.9], size=(n, 1, 3))
    small = sio._tris_from((c + rng.uniform(-0.02, 0.02, size=(n, 3, 3))).reshape(n, 9).astype(np.float32), [(0.5, 0.5, 0.5, 1.0, 0.0, 0.0)] * n)
    same = sio._tris_from([(-0.45, -0.3, 0.5, 0.15, -0.3, 0.55, -0.15, 0.4, 0.5)] * copies,
                          [(0.9 if k % 2 == 0 else 0.1, 0.1 + 0.08 * k, 0.9 if k % 2 else 0.1, 1.0, 0.0, 0.0) for k in range(copies)])
    tr = np.concatenate([small[:150], same, small[150:]])
    tr["id"] = np.arange(len(tr))
    first = len(sp) + len(L) + 150                   # ordinal of the first copy: spheres, then light balls, then triangles
    return (L, sp, tr, _cam(64, 48), 64, 48, 3, 3, dict(seed=17, samples_per_pass=3)), list(range(first, first + copies))


def leaves_of(tree):
    """ordinal -> (first triangle slot of its leaf, node steps from the root to that leaf) in an exported tree."""
    out, todo = {}, [(0, 0)]
    while todo:
        node, depth = todo.pop()
        for code in tree["qnodes"][node, 6:8]:
            code = int(code)
            if code >= 0xFFFFFFFE:                   # empty child
                continue
            if code & 0x80000000:
                first, cnt = (code & 0x7FFFFFFF) >> 3, (code & 7) + 1
                for k in range(first, first + cnt):
                    out[int(tree["tris"][k, 3])] = (first, depth + 1)
            else:
                todo.append((code, depth + 1))
    return out


@pytest.mark.parametrize("copies", [2, 10])
def test_ties(hpt, oracle_mod, copies):
    args, ordinals = ties_case(copies)
    L, sp, tr = args[:3]
    where = leaves_of(hpt.export_bvh_host(L, sp, tr))
    leaves = sorted({where[o] for o in ordinals})
    print("%d copies in leaves (first slot, node steps below the root): %s" % (copies, leaves))
    assert min(d for _, d in leaves) <= 3                              # a ray with three node steps gets to a copy
    if copies == 10:
        assert len(leaves) >= 2                                        # ... and finds the others after it was set aside
    ref, st = pc.oracle_render(oracle_mod, args)
    assert pc.lit_share(ref) > 0.05                                  # the copies fill an eleventh of the view
    # the ordinal decides: the same scene with the copies' materials in reverse order is another image
    lo, hi = ordinals[0] - len(sp) - len(L), ordinals[-1] + 1 - len(sp) - len(L)
    swapped = tr.copy()
    swapped["mtl"][lo:hi] = tr["mtl"][lo:hi][::-1]
    other, _ = pc.oracle_render(oracle_mod, args[:2] + (swapped,) + args[3:])
    assert not np.array_equal(other, ref)
    with hpt.Scene(L, sp, tr) as scene:
        images = {"unsplit": _render(hpt, scene, args, NO_SPLIT)}
        for budget in (1, 2, 3, 0):
            images["budget %d" % budget] = _render(hpt, scene, args, budget)
        images["budget 3, passes of 1"] = _render(hpt, scene, args, 3, samples_per_pass=1)
    _check(images, ref)


# ---- iteration 0 next to the others -------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2])
def test_iteration_0_next_to_the_others(hpt, oracle_mod, depth):
    args = _ball_box(64, 64, 4, depth=depth, seed=8)
    ref, st = pc.oracle_render(oracle_mod, args)
    assert ref.any()
    images = {}
    with hpt.Scene(*args[:3]) as scene:
        for what, budget in (("unsplit", NO_SPLIT), ("default budget", 0), ("budget 1", 1)):
            images[what] = _render(hpt, scene, args, budget)
            images[what + ", passes of 1"] = _render(hpt, scene, args, budget, samples_per_pass=1)
        # two pipelines: each with record arrays of its own
        images["budget 1, two passes in flight"] = _render(hpt, scene, args, 1, samples_per_pass=2)
    _check(images, ref)


# ---- strided launches ---------------------------------------------------------------------------------------------------
STRIDED_W = STRIDED_H = 1024
STRIDED_SPP = 6
STRIDED_WINDOW = (700, 210, 764, 274)         # 64 x 64 over the upper right edge of the ball (columns 496 to 752, rows 224 to 480)
BLIND_GROUPS, LONG_CHUNK = 8 * 256, 2048      # render_pt.cpp: 8 workgroups per CU (256 on the MI355X); kTraceChunk


def strided_case():
    """cornell_with_sphere(2000) with every wall but the floor a perfect mirror, eye depth 1: a path is alive past iteration 0
    exactly while it has met nothing but mirrors; the ball and the floor end it."""
    L, sp, tr = sio.cornell_with_sphere(2000)
    tr = tr.copy()
    tr["mtl"]["base_color"][2:N_WALLS] = 1.0
    tr["mtl"]["roughness"][2:N_WALLS] = 0.0
    tr["mtl"]["metallic"][2:N_WALLS] = 1.0
    tr["mtl"]["type"][2:N_WALLS] = 2
    return L, sp, tr, _cam(STRIDED_W, STRIDED_H), STRIDED_W, STRIDED_H, 1, STRIDED_SPP, dict(seed=9, max_delta=4, samples_per_pass=STRIDED_SPP)


def test_strided_launches(hpt, oracle_mod):
    args = strided_case()
    L, sp, tr, cam, W, H, depth, spp, kw = args
    # share of the primary rays whose first hit is a mirror (64 x 64 sample of the image plane): they are the queue of
    # iteration 1, which has to hold more 2048-ray chunks than the capped grid has workgroups
    small = _cam(64, 64)
    dirs = pc.primary_dirs(small, 64, 64).reshape(-1, 3)
    org = np.tile(np.asarray(small["eye"], np.float32).reshape(1, 3), (len(dirs), 1))
    tri = np.asarray(oracle_mod.closest_hits(L, sp, tr, org, dirs)[1]) - (len(sp) + len(L))
    mirror = float(((tri >= 2) & (tri < N_WALLS)).mean())
    alive = mirror * W * H * spp
    print("primary rays that meet a mirror: %.1f %%: about %.0f rays in iteration 1, %d fill the capped grid" % (100.0 * mirror, alive, BLIND_GROUPS * LONG_CHUNK))
    assert alive > 1.05 * BLIND_GROUPS * LONG_CHUNK
    ref, st = pc.oracle_render(oracle_mod, args, window=STRIDED_WINDOW)
    x0, y0, x1, y1 = STRIDED_WINDOW
    assert st["delta_bounces"] > 0 and 0.2 < pc.lit_share(ref[y0:y1, x0:x1])
    with hpt.Scene(L, sp, tr) as scene:
        images = {"host looks": _render(hpt, scene, args),
                  "blind tail": _render(hpt, scene, args, flags=hpt.FLAG_NO_HOST_WAIT),
                  "blind tail, budget 1": _render(hpt, scene, args, 1, flags=hpt.FLAG_NO_HOST_WAIT),
                  "host looks, unsplit": _render(hpt, scene, args, NO_SPLIT)}
    _check(images, ref, STRIDED_WINDOW)


# ---- two ranks' tiles ---------------------------------------------------------------------------------------------------
def test_two_ranks(hpt, oracle_mod):
    import torch
    W, H, tile, world, spp = 50, 37, 8, 2, 3
    args = _ball_box(W, H, spp, seed=15)
    L, sp, tr, cam = args[:4]
    kw = args[8]
    ref, st = pc.oracle_render(oracle_mod, args)
    assert ref.any()
    stream = torch.cuda.current_stream().cuda_stream
    n_local = hpt.local_pixels(W, H, hpt.make_params(world=world, tile=tile))
    assert n_local != W * H and (-(-W // tile) * -(-H // tile)) % world == 1          # rank 0 owns one tile more
    images = {}
    with hpt.Scene(L, sp, tr) as scene:
        images["one device, unsplit"] = _render(hpt, scene, args, NO_SPLIT, tile=tile)
        for what, budget, more in (("two ranks", 0, {}), ("two ranks, budget 1", 1, {}), ("two ranks, budget 1, passes of 1", 1, dict(samples_per_pass=1))):
            gathered = torch.full((world, n_local, 3), 7.0, dtype=torch.float32, device="cuda")
            for r in range(world):
                scene.render_pt_device(cam, W, H, 4, spp, _params(hpt, kw, budget, rank=r, world=world, tile=tile, **more), gathered[r].data_ptr(), stream)
            image = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            hpt.untile(gathered.data_ptr(), image.data_ptr(), W, H, hpt.make_params(world=world, tile=tile), stream)
            torch.cuda.synchronize()
            images[what] = image.cpu().numpy()
            assert not (gathered.cpu().numpy() == 7.0).any()
    _check(images, ref)


# ---- workspace growth ---------------------------------------------------------------------------------------------------
def test_workspace_growth(hpt, oracle_mod):
    small, big = _ball_box(64, 64, 4), _ball_box(256, 256, 4)
    ref, st = pc.oracle_render(oracle_mod, small)
    assert ref.any()
    for budget in (0, 1):
        with hpt.Scene(*small[:3]) as scene:
            first = _render(hpt, scene, small, budget)
            grown = _render(hpt, scene, big, budget)
            third = _render(hpt, scene, small, budget)
            unsplit = _render(hpt, scene, big, NO_SPLIT)
        print("budget %d: %d pixels of the third render differ from the first, %d of the first from the oracle" % (
            budget, int((third != first).any(axis=-1).sum()), int((first != ref).any(axis=-1).sum())))
        assert np.array_equal(first, ref) and np.array_equal(third, first)
        assert np.isfinite(grown).all() and np.array_equal(grown, unsplit)
