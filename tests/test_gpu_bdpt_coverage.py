"""The bidirectional (cpu_bdpt-estimator) path on the MI355X against the CPU oracle at the cases of bdpt_cases.py:
unequal eye and light depths, light-vertex counts off the 8-entry and 64-vertex tiles of k_bdpt_reduce and
k_bdpt_connect, per-group trees deeper than 12 levels, scattered / sphere-only / flat groups with ties across them, a
parallel light that arrives, a low delta cap, edge scenes and a scene far from the origin -- plus what the host loop
keeps between renders (the grouped scene, the workspace tables) and its argument checks.

Every comparison with the oracle is the project's stated bar (RMSE < 1e-3, max-abs <= 1e-6) and, beyond it, bytes;
with FLAG_COUNT_WORK the shadow rays of the connection stage are the connections the oracle counted.
tests/test_bdpt_cases_cpu.py keeps the oracle images of these cases from being black."""
import numpy as np
import pytest

import bdpt_cases as bc
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


def _camera(sio, args):
    eye, look, up, fov = args[4]
    return sio.make_camera(eye, look, up, fov, args[5], args[6], tan_in_float=True)


def _render(hpt, scene, cam, args, **params):
    L, sp, tr, order, _, W, H, ed, ld, spp, spl, seed, max_delta = args
    return scene.render_bdpt(cam, W, H, ed, ld, spp, spl, hpt.make_params(seed=seed, max_delta=max_delta, **params))


def bdpt_parity(hpt, sio, args, ref, ref_stats):
    """Three renders of one grouped scene -- counting work, plain, and one sample per pass in 8 x 8 tiles -- are the
    oracle's image, and the counted connection work is consistent with the oracle's count."""
    L, sp, tr, order = args[:4]
    cam = _camera(sio, args)
    with hpt.Scene(L, sp, tr) as scene:
        scene.set_groups(*order)
        counted = _render(hpt, scene, cam, args, flags=hpt.FLAG_COUNT_WORK)
        st = scene.stats()
        plain = _render(hpt, scene, cam, args)
        passes = _render(hpt, scene, cam, args, samples_per_pass=1, tile=8)
    for what, img in (("counted", counted), ("plain", plain), ("one sample per pass", passes)):
        d = np.abs(img - ref)
        print("%s: max abs %.3e, differing pixels %d" % (what, float(d.max()) if d.size else 0.0, int((img != ref).any(axis=-1).sum())))
    print("stats: pairs %d survivors %d shadow rays %d unoccluded %d; oracle connections %d" % (
        st["bd_pairs"], st["bd_survivors"], st["bd_shadow_rays"], st["bd_unoccluded"], ref_stats["connections"]))
    for img in (counted, plain, passes):
        assert_parity(img, ref)
        assert np.array_equal(img, ref)
    n_lv = bc.n_light_vertices(args)
    assert st["bd_shadow_rays"] == ref_stats["connections"]
    assert st["bd_pairs"] % max(n_lv, 1) == 0
    assert st["bd_pairs"] >= st["bd_survivors"] >= st["bd_shadow_rays"] >= st["bd_unoccluded"]
    return plain, st


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_case_matches_the_oracle(hpt, sio, oracle_mod, name):
    args, ref, ref_stats = bc.reference(oracle_mod, name)
    if name.startswith("deep-"):
        assert hpt.export_bvh_host(*args[:3])["bvh_depth"] > 12          # the group's tree comes from the same builder
    img, st = bdpt_parity(hpt, sio, args, ref, ref_stats)
    if name in bc.ALL_ZERO:
        assert not img.any() and st["bd_pairs"] == 0


@pytest.mark.parametrize("seed", bc.GROUP_SEEDS)
def test_groups_take_effect_after_a_render(hpt, sio, oracle_mod, seed):
    """hpt_scene_set_groups after a first render drops the device scene of the bidirectional path; the next render builds
    the grouped one, and handing over no objects goes back to the single implicit group."""
    args, grouped_ref, _ = bc.reference(oracle_mod, "groups-%d" % seed)
    L, sp, tr, order = args[:4]
    one = list(args); one[3] = bc.single_group(sp, tr)
    single_ref, _ = bc.oracle_render(oracle_mod, tuple(one))
    assert not np.array_equal(single_ref, grouped_ref)
    cam = _camera(sio, args)
    none = np.zeros(0, np.int32)
    with hpt.Scene(L, sp, tr) as scene:
        a = _render(hpt, scene, cam, args)
        scene.set_groups(*order)
        b = _render(hpt, scene, cam, args)
        scene.set_groups(none, none, none)
        c = _render(hpt, scene, cam, args)
        scene.set_groups(*order)
        d = _render(hpt, scene, cam, args)
    assert np.array_equal(a, single_ref) and np.array_equal(b, grouped_ref)
    assert np.array_equal(c, single_ref) and np.array_equal(d, grouped_ref)


def test_workspace_reuse_across_shapes(hpt, sio, oracle_mod):
    """One scene rendered at shapes that grow and shrink each of the workspace's tables (path slots, eye_depth x slots
    history, slots x n_lv contributions, n_lv light vertices), with a PT and a photon-mapping render in between, gives
    what a fresh scene gives for the same call."""
    sc, L, sp, tr, order = bc._input()
    eye, look, up, fov = bc._input_cam(sc)
    shapes = {"A": (48, 36, 4, 3, 2, 5), "B": (24, 20, 2, 7, 2, 13), "C": (64, 48, 6, 1, 2, 1)}      # W, H, eye, light, spp, spl

    def bd(scene, key, **params):
        W, H, ed, ld, spp, spl = shapes[key]
        cam = sio.make_camera(eye, look, up, fov, W, H, tan_in_float=True)
        return scene.render_bdpt(cam, W, H, ed, ld, spp, spl, hpt.make_params(seed=8, **params))

    def pt(scene):
        return scene.render_pt(sio.camera_for(sc, 40, 30), 40, 30, 4, 2, hpt.make_params(seed=8))

    def ppm(scene):
        return scene.render_ppm(sio.camera_for(sc, 40, 30), 40, 30, 4, 4, 1, 64, 0.05, hpt.make_params(seed=8))

    steps = [("A", lambda s: bd(s, "A")), ("B", lambda s: bd(s, "B")), ("pt", pt), ("C", lambda s: bd(s, "C")), ("ppm", ppm),
             ("A1", lambda s: bd(s, "A", samples_per_pass=1)), ("B", lambda s: bd(s, "B"))]
    fresh = {}
    for key, call in steps:
        if key not in fresh:
            with hpt.Scene(L, sp, tr) as scene:
                scene.set_groups(*order)
                fresh[key] = call(scene)
    with hpt.Scene(L, sp, tr) as scene:
        scene.set_groups(*order)
        reused = [(key, call(scene)) for key, call in steps]
    for k, (key, img) in enumerate(reused):
        assert np.array_equal(img, fresh[key]), (k, key)
    assert np.array_equal(fresh["A"], fresh["A1"])
    W, H, ed, ld, spp, spl = shapes["A"]
    ref, _ = oracle_mod.bdpt_render(L, sp, tr, order, eye, look, up, fov, W, H, ed, ld, spp, spl, seed=8)
    assert ref.mean() > 0.01
    assert_parity(fresh["A"], ref)
    assert np.array_equal(fresh["A"], ref)


def test_sample_offset_and_output_sum(hpt, sio, oracle_mod):
    """Progressive accumulation on the host: samples 0-2 and 3-6 as sums add up to the 7-sample mean (the PT test's
    bounds); every part is the oracle's, which has no sample offset: its 7-sample image is compared with the whole."""
    sc, L, sp, tr, order = bc._input()
    eye, look, up, fov = bc._input_cam(sc)
    W, H, ed, ld, spl = 40, 28, 3, 5, 3
    cam = sio.make_camera(eye, look, up, fov, W, H, tan_in_float=True)
    with hpt.Scene(L, sp, tr) as scene:
        scene.set_groups(*order)
        whole = scene.render_bdpt(cam, W, H, ed, ld, 7, spl, hpt.make_params(seed=9))
        s0 = scene.render_bdpt(cam, W, H, ed, ld, 3, spl, hpt.make_params(seed=9, flags=hpt.FLAG_OUTPUT_SUM))
        s1 = scene.render_bdpt(cam, W, H, ed, ld, 4, spl, hpt.make_params(seed=9, sample_offset=3, flags=hpt.FLAG_OUTPUT_SUM))
        m0 = scene.render_bdpt(cam, W, H, ed, ld, 3, spl, hpt.make_params(seed=9))
    ref, _ = oracle_mod.bdpt_render(L, sp, tr, order, eye, look, up, fov, W, H, ed, ld, 7, spl, seed=9)
    ref3, _ = oracle_mod.bdpt_render(L, sp, tr, order, eye, look, up, fov, W, H, ed, ld, 3, spl, seed=9)
    assert np.array_equal(whole, ref) and np.array_equal(m0, ref3)
    assert whole.mean() > 0.01 and not np.array_equal(s0, s1)
    assert np.allclose(s0 / 3.0, m0, rtol=1e-6, atol=1e-7)                 # the same sums, one division apart
    assert np.allclose((s0 + s1) / 7.0, whole, rtol=1e-5, atol=1e-6)


def test_virtual_ranks_with_unequal_depths(hpt, sio, oracle_mod):
    """test_bdpt_virtual_ranks_assemble_bitwise at depths 2 / 5: the history tables of a rank are strided by its own
    slot count, the light subpaths are every rank's own copy."""
    import torch
    sc, L, sp, tr, order = bc._input()
    eye, look, up, fov = bc._input_cam(sc)
    W, H, spp, spl = 52, 40, 2, 3
    cam = sio.make_camera(eye, look, up, fov, W, H, tan_in_float=True)
    stream = torch.cuda.current_stream().cuda_stream
    with hpt.Scene(L, sp, tr) as scene:
        scene.set_groups(*order)
        ref = scene.render_bdpt(cam, W, H, 2, 5, spp, spl, hpt.make_params(seed=21))
        assert ref.mean() > 0.01
        for world, tile in ((3, 16), (8, 8)):
            n_local = hpt.local_pixels(W, H, hpt.make_params(world=world, tile=tile))
            gathered = torch.zeros((world, n_local, 3), dtype=torch.float32, device="cuda")
            for r in range(world):
                p = hpt.make_params(seed=21, rank=r, world=world, tile=tile)
                scene.render_bdpt_device(cam, W, H, 2, 5, spp, spl, p, gathered[r].data_ptr(), stream)
            image = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            hpt.untile(gathered.data_ptr(), image.data_ptr(), W, H, hpt.make_params(world=world, tile=tile), stream)
            torch.cuda.synchronize()
            assert np.array_equal(image.cpu().numpy(), ref), "world=%d" % world


def test_argument_errors(hpt, sio):
    """Counts and depths out of range, more than 2^24 light vertices and a contribution table over 64 GiB are
    HPT_ERR_INVALID before anything is allocated for them; the scene renders on unchanged."""
    sc, L, sp, tr, order = bc._input()
    assert len(L) == 4
    eye, look, up, fov = bc._input_cam(sc)
    cam = sio.make_camera(eye, look, up, fov, 24, 20, tan_in_float=True)
    big = sio.make_camera(eye, look, up, fov, 2048, 2048, tan_in_float=True)
    with hpt.Scene(L, sp, tr) as scene:
        scene.set_groups(*order)
        good = scene.render_bdpt(cam, 24, 20, 3, 2, 2, 3, hpt.make_params(seed=5))
        assert good.mean() > 0.01
        for c, W, H, ed, ld, spp, spl in ((cam, 24, 20, 3, 2, 2, 0),                   # spl 0
                                          (cam, 24, 20, 0, 2, 2, 3), (cam, 24, 20, 3, 0, 2, 3),          # depth 0
                                          (cam, 24, 20, 256, 2, 2, 3), (cam, 24, 20, 3, 256, 2, 3),      # depth 256
                                          (cam, 24, 20, 3, 5, 2, 1 << 20),              # 4 * 2^20 * 5 light vertices > 2^24
                                          (big, 2048, 2048, 3, 4, 1, 100)):             # 4 Mi slots x 1600 x 16 B = 100 GiB
            with pytest.raises(hpt.HptError, match="hpt error 1:"):
                scene.render_bdpt(c, W, H, ed, ld, spp, spl, hpt.make_params(seed=5))
            assert np.array_equal(scene.render_bdpt(cam, 24, 20, 3, 2, 2, 3, hpt.make_params(seed=5)), good)
