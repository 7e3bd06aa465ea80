"""Bounded device builds on the MI355X (include/hpt.h, "bounded device builds"): hpt_scene_rebuild_device_bounded on every pair
of bounded_cases.py, the depths of one case on one handle.  The order inside a pair shows a wrong tree before anything walks
it: the exported tree, both info records and the cost kernel's sums are held to the host definition
(hpt_bvh_device_build_bounded_host) first; then the path tracer and the probes must return the bytes they returned before
any build; then an update refits the new topology.  An unbounded device build between the depths is held to its own
definition.  What a bounded build leaves alone is shown against a twin handle that did not rebuild.  Every render is
32 x 24, 2 spp."""
import collections
import os
import re

import numpy as np
import pytest

import bounded_cases as bcs
import bounded_oracle as bo
import device_build_cases as dc
import skin_cases as sc
from path_tracing_amd import scene_io as sio
from test_gpu_device_build import BUILD_KEYS, MOTION_KEYS, _cli, _probes, _pt, _same_tree, _tree_is_the_definition
from test_gpu_refit import _probe_rays, _same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
WALKS = (("default", 0, 0), ("budget 63: no split", 0, 63), ("budget 1: the resume launch's wide tree", 0, 1))
DEPTHS = collections.OrderedDict()
for _name, _d in bcs.ALL_PAIRS:
    DEPTHS.setdefault(_name, []).append(_d)


def _built_is_the_definition(hpt, scene, L, sp, tr, want, what, builds, before):
    """Export, cost and both records against the definition `want`; where it says the build falls back, the host builder's tree."""
    fell_back = want["build"]["fell_back"]
    dev = _tree_is_the_definition(hpt, scene, hpt.export_bvh_host(L, sp, tr) if fell_back else want, what)
    di, bi, st = scene.device_build_info(), scene.bounded_build_info(), scene.stats()
    assert bi == want["bounded"], (what, bi)
    assert di["builds"] == builds and di["fell_back"] == fell_back, (what, di)
    if not fell_back:
        assert {k: di[k] for k in BUILD_KEYS} == {k: want["build"][k] for k in BUILD_KEYS}, (what, di)
        assert dev["bvh_depth"] <= bi["max_depth"], what
    assert (di["nodes_before"], di["depth_before"]) == before, (what, di)
    assert (st["bvh_nodes"], st["bvh_depth"]) == (dev["num_nodes"], dev["bvh_depth"]) == (di["nodes_after"], di["depth_after"]), what
    return di


@pytest.mark.parametrize("name", list(DEPTHS))
def test_case(hpt, name):
    L, sp, tr = bcs.records(name)
    rays = _probe_rays(tr, 7)
    depths = DEPTHS[name]
    with hpt.Scene(L, sp, tr) as scene:
        # 1. before any build
        img = _pt(hpt, scene)
        probes = _probes(scene, rays)
        assert scene.bounded_build_info() == dict(max_depth=0, forced_nodes=0, first_forced_level=0)
        plain = dc.tree(hpt, name) if name in dc.CASES else hpt.device_build_bvh_host(L, sp, tr)
        builds = 0
        for k, depth in enumerate(depths):
            what = "%s at %d" % (name, depth)
            want = bcs.tree(hpt, name, depth)
            st = scene.stats()
            # 2. the build: the definition's bytes, its records, the cost kernel's sums -- before anything walks the tree
            scene.rebuild_device_bounded(depth)
            builds += 1
            di = _built_is_the_definition(hpt, scene, L, sp, tr, want, what + " built", builds, (st["bvh_nodes"], st["bvh_depth"]))
            assert scene.update_info()["updates"] == (2 if k else 0)              # (step 4's two, after the first depth)
            _same(what + ": the records are untouched", scene.read_triangles(), tr)
            print("%s: %d triangles, nodes %d, depth %d, wide depth %d, forced %d from level %d; sort %.3f topology %.3f refit %.3f collapse %.3f ms"
                  % (what, len(tr), di["nodes_after"], di["depth_after"], di["wide_depth"], want["bounded"]["forced_nodes"],
                     want["bounded"]["first_forced_level"], di["ms_sort"], di["ms_topology"], di["ms_refit"], di["ms_collapse"]))
            # 3. the image and the probes do not depend on the tree
            for walk, flags, budget in (WALKS if name not in dc.BIG else WALKS[:1]):
                _same("%s built: render_pt, %s" % (what, walk), _pt(hpt, scene, flags, budget), img)
            for j, (got, was) in enumerate(zip(_probes(scene, rays), probes)):
                _same("%s built: probe %d" % (what, j), got, was)
            if k == 0:
                # 4. an update refits the new topology; and back
                scene.update_triangles(dc.moved(tr))
                _tree_is_the_definition(hpt, scene, hpt.device_build_bounded_bvh_host(L, sp, tr, scene.read_triangles(), depth), what + " built, then moved")
                scene.update_triangles(tr)
                _same_tree(what + ": back on the build's records", scene.export_bvh(), hpt.export_bvh_host(L, sp, tr) if want["build"]["fell_back"] else want)
                # 5. an unbounded device build on the same handle gives its own definition (deep63: the host builder's tree)
                scene.rebuild_device()
                builds += 1
                _tree_is_the_definition(hpt, scene, hpt.export_bvh_host(L, sp, tr) if plain["build"]["fell_back"] else plain, what + ", then unbounded")
                assert scene.device_build_info()["builds"] == builds and scene.device_build_info()["fell_back"] == plain["build"]["fell_back"]
                assert scene.bounded_build_info() == want["bounded"]          # the last bounded build's, still
                _same(what + ", then unbounded: render_pt", _pt(hpt, scene), img)
        # host rebuilds: the fallbacks alone, as the definitions decide them
        assert scene.rebuild_info()["rebuilds"] == plain["build"]["fell_back"] + sum(bcs.tree(hpt, name, d)["build"]["fell_back"] for d in depths)


def test_deep63_builds_on_the_device(hpt):
    """Where hpt_scene_rebuild_device falls back (61 levels), the bounded build at the limit does not."""
    L, sp, tr = bcs.records("deep63")
    want = bcs.tree(hpt, "deep63", 0)
    assert dc.tree(hpt, "deep63")["build"]["fell_back"] == 1 and want["build"]["fell_back"] == 0
    with hpt.Scene(L, sp, tr) as scene:
        scene.rebuild_device_bounded(0)
        di, bi = scene.device_build_info(), scene.bounded_build_info()
        assert di["fell_back"] == 0 and scene.rebuild_info()["rebuilds"] == 0 and di["ms_topology"] > 0.0
        assert di["depth_after"] <= 30 and bi["forced_nodes"] > 0 and bi["max_depth"] == 30
        _same_tree("deep63 at 0", scene.export_bvh(), want)


# ---- what a bounded build leaves alone: a twin handle that does not rebuild ---------------------------------------------

def test_state_across_a_bounded_build(hpt):
    """test_gpu_device_build's twins (skin_cases' bend: groups, a skin two steps in with the previous geometry kept, the lazy
    structures built, an hpt_sppm state two passes in); one twin builds at need + 1, which forces nodes."""
    d = sc.data("bend")
    cam = sc.camera("bend")
    bcam = sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, sc.W, sc.H, tan_in_float=True)
    kw = dict(eye_depth=4, light_depth=4, spl=256, radius=0.07)
    depth = bo.need(len(d.tr)) + 1

    def renders(scene):
        g = scene.render_guides(cam, sc.W, sc.H, 2, hpt.make_params(seed=7), prev_position=True)
        return [scene.render_bdpt(bcam, sc.W, sc.H, 4, 4, 2, 8, hpt.make_params(seed=3)),
                scene.render_ppm(cam, sc.W, sc.H, 4, 4, 1, 256, 0.07, hpt.make_params(seed=5))] + [g[k].view(np.uint32) for k in MOTION_KEYS]

    with hpt.Scene(d.L, d.sp, d.tr) as a, hpt.Scene(d.L, d.sp, d.tr) as b:
        states = []
        try:
            for s in (a, b):
                s.set_groups(*d.order)
                s.set_skin(*d.steps[0][1:])
                s.skin(d.steps[1][1])
                s.keep_previous()
                s.skin(d.steps[2][1])
                states.append(s.sppm(cam, sc.W, sc.H, alpha=0.7, params=hpt.make_params(seed=5), **kw))
                states[-1].render(2)
            before = renders(a)
            info, at_build = a.update_info(), a.read_triangles()
            a.rebuild_device_bounded(depth)
            want = hpt.device_build_bounded_bvh_host(d.L, d.sp, at_build, None, depth)
            assert a.device_build_info()["builds"] == 1 and a.device_build_info()["fell_back"] == 0 and b.device_build_info()["builds"] == 0
            assert a.bounded_build_info() == want["bounded"] and want["bounded"]["forced_nodes"] > 0 and b.bounded_build_info()["max_depth"] == 0
            _same_tree("bend built", a.export_bvh(), want)
            assert a.update_info() == info and a.has_motion() == b.has_motion() and a.rebuild_info()["rebuilds"] == 0
            for k, (x, y, z) in enumerate(zip(renders(a), renders(b), before)):
                _same("bend built: render %d against the twin" % k, x, y)
                _same("bend built: render %d against itself before" % k, x, z)
            _same("SPPM passes 3 and 4", states[0].render(2), states[1].render(2))
            sa, sb = states[0].state(), states[1].state()
            assert sa["passes"] == sb["passes"] == 4
            _same("SPPM radius", sa["radius2"], sb["radius2"])
            _same("SPPM photons", sa["photons"], sb["photons"])
            for s in (a, b):
                s.skin(d.steps[3][1])
            moved = b.read_triangles()
            _same("bend: the records after the next step", a.read_triangles(), moved)
            _same_tree("bend: the next step refits the new topology", a.export_bvh(), hpt.device_build_bounded_bvh_host(d.L, d.sp, at_build, moved, depth))
            for k, (x, y) in enumerate(zip(renders(a), renders(b))):
                _same("bend, the next step: render %d against the twin" % k, x, y)
        finally:
            for p in states:
                p.close()


def test_refusals_leave_the_handle_as_it_was(hpt):
    lib = hpt.load_library()
    for name in sorted({n for n, _ in bcs.REFUSED}):
        L, sp, tr = bcs.records(name)
        with hpt.Scene(L, sp, tr) as scene:
            img, tree = _pt(hpt, scene), scene.export_bvh()
            for depth in [d for n, d in bcs.REFUSED if n == name]:
                with pytest.raises(hpt.HptError) as e:
                    scene.rebuild_device_bounded(depth)
                assert str(e.value).startswith("hpt error 1:") and "max_depth" in str(e.value)
            assert lib.hpt_scene_rebuild_device_bounded(None, 0) == 1 and b"null scene" in lib.hpt_last_error()
            assert lib.hpt_scene_get_bounded_build_info(scene._h, None) == 1 and b"null" in lib.hpt_last_error()
            if hpt.device_count() >= 2:
                import torch
                torch.cuda.set_device(1)
                try:
                    with pytest.raises(hpt.HptError) as e:
                        scene.rebuild_device_bounded(0)
                    assert str(e.value).startswith("hpt error 1:") and "another device" in str(e.value)
                finally:
                    torch.cuda.set_device(0)
            assert scene.device_build_info() == {k: 0 for k in scene.device_build_info()}
            assert scene.bounded_build_info() == {k: 0 for k in scene.bounded_build_info()}
            _same_tree(name + " after the refusals", scene.export_bvh(), tree)
            _same(name + " after the refusals: render_pt", _pt(hpt, scene), img)


# ---- CLI -----------------------------------------------------------------------------------------------------------------

def test_cli_rebuild_depth_keeps_the_image(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    obj = str(tmp_path / "mesh.obj")
    sio.write_obj(obj, sio._tris_from(sio.tessellated_sphere((-0.15, 0.25, 0.0), 0.15, 12, 12), np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), np.float32), (264, 1))))
    base = ["--mode", "pt", "--input", scene_file, "--obj", obj, "--seed", 13, "--width", 64, "--height", 48, "--frame-spp", 2, "--guide-spp", 3,
            "--frames", 3, "--twist-device", 5, "--reproject"]
    plain = _cli(*base, "--output", tmp_path / "plain.png")
    assert plain.returncode == 0 and "[Success] Image saved!" in plain.stdout and "[Rebuild]" not in plain.stdout, plain.stdout + plain.stderr
    run = _cli(*base, "--output", tmp_path / "built.png", "--rebuild-device", "--rebuild-depth", 8)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    lines = re.findall(r"^\[Rebuild\] frame (\d+) device nodes (\d+) depth (\d+) (\S+) ms$", run.stdout, flags=re.M)
    assert [int(f) for f, _, _, _ in lines] == [1, 2], run.stdout                # before every frame that follows an update, never "host"
    assert all(int(n) > 1 and 1 <= int(d) <= 8 and float(ms) > 0.0 for _, n, d, ms in lines)
    frames = lambda text: re.findall(r"^\[Frame \d+\].*$", text, flags=re.M)
    assert frames(run.stdout) == frames(plain.stdout) and len(frames(run.stdout)) == 3
    with open(tmp_path / "plain.png", "rb") as f, open(tmp_path / "built.png", "rb") as g:
        assert f.read() == g.read()
    for extra, word in ((["--rebuild-depth", 8], "--rebuild-depth needs --rebuild-device"), (["--rebuild-device", "--rebuild-depth", 31], "--rebuild-depth needs 0 or"),
                        (["--rebuild-device", "--rebuild-depth", "x"], "--rebuild-depth needs 0 or"), (["--rebuild-device", "--rebuild-depth", 3], "max_depth")):
        r = _cli(*base, "--output", tmp_path / "y.png", *extra)
        assert r.returncode != 0 and word in r.stderr and not os.path.exists(tmp_path / "y.png"), (extra, r.stdout + r.stderr)
