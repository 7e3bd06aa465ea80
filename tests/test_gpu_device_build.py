"""Device builds on the MI355X (include/hpt.h, "device builds"): hpt_scene_rebuild_device on every case of device_build_cases.py.
The order inside a case shows a wrong tree before anything walks it: the exported tree is held to the bytes of the host
definition (hpt_bvh_device_build_host) and measured by the cost kernel first, then the path tracer and the probes must return
the bytes they returned before the build under every way the tree is walked, then every kind of update refits the new
topology, and a host rebuild and a second device build give their own bytes again.  What a device build leaves alone is shown
against a twin handle that did not rebuild.  Every render is 32 x 24, 2 spp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cost_oracle as co
import device_build_cases as dc
import refit_cases as rc
import skin_cases as sc
from path_tracing_amd import scene_io as sio
from test_gpu_refit import TREE_KEYS, _params, _probe_rays, _same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "path_tracing_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")
BUILD_KEYS = ("fell_back", "nodes_after", "depth_after", "wide_depth")
MOTION_KEYS = ("albedo", "normal", "position", "coverage", "prev_position")
WALKS = (("default", 0, 0), ("budget 63: no split", 0, 63), ("budget 1: the resume launch's wide tree", 0, 1), ("counting", None, 0))


def _pt(hpt, scene, flags=0, budget=0):
    return scene.render_pt(dc.camera(), dc.W, dc.H, dc.DEPTH, dc.SPP, _params(hpt, flags, budget, seed=dc.SEED))


def _same_tree(what, got, want):
    for k in TREE_KEYS:
        _same("%s: exported %s" % (what, k), got[k], want[k])


def _probes(scene, rays):
    o, d, p2 = rays
    t, prim = scene.trace_closest(o, d)
    return t, prim, scene.trace_visibility(o, p2)


def _tree_is_the_definition(hpt, scene, want, what):
    """Export, info and cost, before anything walks the tree."""
    dev = scene.export_bvh()
    _same_tree(what, dev, want)
    got, host = scene.tree_cost(), hpt.tree_cost_host(dev)
    co.same(what + ": cost", got, host)
    assert got["bytes"] == host["bytes"], what
    assert got["leaf_slots"] == dev["num_tris"] and got["inner_children"] + 1 == dev["num_nodes"], what
    return dev


def _updates(hpt, scene, tr):
    """(name, call) of one update of every kind, each on the geometry the one before left."""
    nt = len(tr)
    rng = np.random.default_rng(11)
    turn = np.array([[0.96, -0.28, 0.0, 0.02], [0.28, 0.96, 0.0, -0.01], [0.0, 0.0, 1.0, 0.03]], np.float32)
    lift = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.04], [0.0, 0.0, 1.0, 0.0]], np.float32)
    bone = np.zeros((nt, 3, 4), np.int32)
    bone[:, :, 1] = 1
    weight = np.zeros((nt, 3, 4), np.float32)
    weight[:, :, 0], weight[:, :, 1] = 0.75, 0.25
    corners = np.arange(0, 3 * nt, 2, dtype=np.int32)
    delta = rng.uniform(-0.03, 0.03, (len(corners), 3)).astype(np.float32)

    def pose():
        scene.set_parts(None, 1)
        scene.pose(turn[None])

    def skin():
        scene.set_skin(bone, weight, 2)
        scene.skin(np.stack([turn, lift]))

    def morph():
        scene.set_morphs(np.array([0, len(corners)], np.int32), corners, delta)
        scene.morph(np.array([0.5], np.float32))

    def device_verts():
        import torch
        v = rc.verts(dc.moved(tr, seed=5)).astype(np.float32)
        scene.update_vertices_device(torch.from_numpy(np.ascontiguousarray(v)).cuda())

    return [("pose", pose), ("skin", skin), ("morph", morph), ("update_triangles", lambda: scene.update_triangles(dc.moved(tr))),
            ("update_vertices_device", device_verts)]


@pytest.mark.parametrize("name", [n for n in dc.NAMES if n not in dc.FALLS_BACK])
def test_case(hpt, name):
    L, sp, tr = dc.records(name)
    want = dc.tree(hpt, name)
    rays = _probe_rays(tr, 7)
    with hpt.Scene(L, sp, tr) as scene:
        # 1. before the build
        img = _pt(hpt, scene)
        probes = _probes(scene, rays)
        before = scene.stats()
        # 2. the build: the definition's bytes, its info, the cost kernel's sums
        scene.rebuild_device()
        dev = _tree_is_the_definition(hpt, scene, want, name + " built")
        di, st = scene.device_build_info(), scene.stats()
        assert {k: di[k] for k in BUILD_KEYS} == {k: want["build"][k] for k in BUILD_KEYS}, di
        assert di["builds"] == 1 and (di["nodes_before"], di["depth_before"]) == (before["bvh_nodes"], before["bvh_depth"])
        assert (st["bvh_nodes"], st["bvh_depth"]) == (dev["num_nodes"], dev["bvh_depth"]) == (di["nodes_after"], di["depth_after"])
        assert (st["n_tris"], st["n_materials"]) == (before["n_tris"], before["n_materials"])
        assert scene.rebuild_info()["rebuilds"] == 0 and scene.update_info()["updates"] == 0 and not scene.has_motion()      # never updated, and still not
        _same(name + ": the records are untouched", scene.read_triangles(), tr)
        print("%s: %d triangles, nodes %d -> %d, depth %d -> %d, wide depth %d; sort %.3f topology %.3f refit %.3f collapse %.3f ms"
              % (name, len(tr), di["nodes_before"], di["nodes_after"], di["depth_before"], di["depth_after"], di["wide_depth"],
                 di["ms_sort"], di["ms_topology"], di["ms_refit"], di["ms_collapse"]))
        # 3. the image and the probes do not depend on the tree
        for what, flags, budget in WALKS:
            _same("%s built: render_pt, %s" % (name, what), _pt(hpt, scene, hpt.FLAG_COUNT_WORK if flags is None else flags, budget), img)
        for k, (got, was) in enumerate(zip(_probes(scene, rays), probes)):
            _same("%s built: probe %d" % (name, k), got, was)
        # 4. every kind of update refits the new topology
        steps = _updates(hpt, scene, tr) if len(tr) else [("update_triangles", lambda: scene.update_triangles(tr))]
        if name in dc.BIG:
            steps = steps[3:4]
        for what, call in steps:
            call()
            now = scene.read_triangles()
            _tree_is_the_definition(hpt, scene, hpt.device_build_bvh_host(L, sp, tr, now), "%s built, then %s" % (name, what))
        scene.update_triangles(tr)                       # back where the build was made
        _same_tree(name + ": back on the build's records", scene.export_bvh(), want)
        _same(name + ": back on the build's records: render_pt", _pt(hpt, scene), img)
        # 5. a host rebuild gives the host builder's bytes again, a second device build the first one's
        scene.rebuild()
        _same_tree(name + ": a host rebuild afterwards", scene.export_bvh(), hpt.export_bvh_host(L, sp, tr))
        assert scene.rebuild_info()["rebuilds"] == 1 and scene.device_build_info()["builds"] == 1
        scene.rebuild_device()
        _tree_is_the_definition(hpt, scene, want, name + " built twice")
        assert scene.device_build_info()["builds"] == 2 and scene.device_build_info()["fell_back"] == 0
        _same(name + " built twice: render_pt", _pt(hpt, scene), img)


# ---- what a device build leaves alone: a twin handle that does not rebuild ----------------------------------------------

def test_state_across_a_device_build(hpt):
    """skin_cases' bend on twins: groups set, a skin two steps in with the previous geometry kept one step back, every lazy
    structure built (a BDPT render, a photon-mapping render with the scene's own bounds) and an hpt_sppm state two passes in.
    One twin builds on the device.  Afterwards both give the same BDPT, photon-mapping, guide (the motion guide with them) and
    SPPM bytes, the same motion flag and update counts, and the next skin step refits the new topology."""
    d = sc.data("bend")
    cam = sc.camera("bend")
    bcam = sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, sc.W, sc.H, tan_in_float=True)
    kw = dict(eye_depth=4, light_depth=4, spl=256, radius=0.07)

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
            a.rebuild_device()
            assert a.device_build_info()["builds"] == 1 and a.device_build_info()["fell_back"] == 0 and b.device_build_info()["builds"] == 0
            _same_tree("bend built", a.export_bvh(), hpt.device_build_bvh_host(d.L, d.sp, at_build))
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
            _same_tree("bend: the next step refits the new topology", a.export_bvh(), hpt.device_build_bvh_host(d.L, d.sp, at_build, moved))
            for k, (x, y) in enumerate(zip(renders(a), renders(b))):
                _same("bend, the next step: render %d against the twin" % k, x, y)
        finally:
            for p in states:
                p.close()


def test_deep63_falls_back_to_the_host_builder(hpt):
    L, sp, tr = dc.records("deep63")
    assert dc.tree(hpt, "deep63")["build"]["fell_back"] == 1
    with hpt.Scene(L, sp, tr) as scene:
        img, tree = _pt(hpt, scene), scene.export_bvh()
        scene.rebuild_device()                            # HPT_OK
        di, ri = scene.device_build_info(), scene.rebuild_info()
        assert di["builds"] == 1 and di["fell_back"] == 1 and ri["rebuilds"] == 1
        assert di["ms_sort"] == di["ms_topology"] == di["ms_refit"] == di["ms_collapse"] == 0.0
        _same_tree("deep63", scene.export_bvh(), hpt.export_bvh_host(L, sp, tr))
        _same_tree("deep63 against the tree it was created with", scene.export_bvh(), tree)
        assert (di["nodes_after"], di["depth_after"]) == (tree["num_nodes"], tree["bvh_depth"]) and di["depth_after"] <= dc.MAX_BVH_DEPTH
        _same("deep63: render_pt", _pt(hpt, scene), img)
        scene.update_triangles(dc.moved(tr))
        _same_tree("deep63, then an update", scene.export_bvh(), hpt.refit_bvh_host(L, sp, tr, scene.read_triangles()))


def test_refusals_leave_the_handle_as_it_was(hpt):
    L, sp, tr = dc.records("edge-257")
    lib = hpt.load_library()
    with hpt.Scene(L, sp, tr) as scene:
        img, tree = _pt(hpt, scene), scene.export_bvh()
        assert lib.hpt_scene_rebuild_device(None) == 1 and b"null scene" in lib.hpt_last_error()
        assert lib.hpt_scene_get_device_build_info(scene._h, None) == 1 and b"null" in lib.hpt_last_error()
        if hpt.device_count() >= 2:
            import torch
            torch.cuda.set_device(1)
            try:
                with pytest.raises(hpt.HptError) as e:
                    scene.rebuild_device()
                assert str(e.value).startswith("hpt error 1:") and "another device" in str(e.value)
            finally:
                torch.cuda.set_device(0)
        assert scene.device_build_info() == {k: 0 for k in scene.device_build_info()}
        _same_tree("after the refusals", scene.export_bvh(), tree)
        _same("after the refusals: render_pt", _pt(hpt, scene), img)


# ---- CLI -----------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(CSRC, "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_rebuild_device_keeps_the_image(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    obj = str(tmp_path / "mesh.obj")
    sio.write_obj(obj, sio._tris_from(sio.tessellated_sphere((-0.15, 0.25, 0.0), 0.15, 12, 12), np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), np.float32), (264, 1))))
    base = ["--mode", "pt", "--input", scene_file, "--obj", obj, "--seed", 13, "--width", 64, "--height", 48, "--frame-spp", 2, "--guide-spp", 3,
            "--frames", 4, "--twist-device", 5, "--reproject"]
    plain = _cli(*base, "--output", tmp_path / "plain.png")
    assert plain.returncode == 0 and "[Success] Image saved!" in plain.stdout and "[Rebuild]" not in plain.stdout, plain.stdout + plain.stderr
    run = _cli(*base, "--output", tmp_path / "built.png", "--rebuild-device")
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    lines = re.findall(r"^\[Rebuild\] frame (\d+) device nodes (\d+) depth (\d+) (\S+) ms$", run.stdout, flags=re.M)
    assert [int(f) for f, _, _, _ in lines] == [1, 2, 3], run.stdout             # before every frame that follows an update
    assert all(int(n) > 1 and 1 <= int(d) <= dc.MAX_BVH_DEPTH and float(ms) > 0.0 for _, n, d, ms in lines)
    frames = lambda text: re.findall(r"^\[Frame \d+\].*$", text, flags=re.M)
    assert frames(run.stdout) == frames(plain.stdout) and len(frames(run.stdout)) == 4
    with open(tmp_path / "plain.png", "rb") as f, open(tmp_path / "built.png", "rb") as g:
        assert f.read() == g.read()
    # with --rebuild-above the policy's rebuilds, if the cost asks for any, are device builds: the "[Rebuild]" lines are the policy's
    run = _cli(*base, "--output", tmp_path / "above.png", "--rebuild-device", "--rebuild-above", 1.0000001)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    assert all(re.match(r"^\[Rebuild\] frame \d+ sah \S+ -> \S+ \S+ ms$", ln) for ln in run.stdout.splitlines() if ln.startswith("[Rebuild]"))
    with open(tmp_path / "plain.png", "rb") as f, open(tmp_path / "above.png", "rb") as g:
        assert f.read() == g.read()
    r = _cli("--mode", "pt", "--input", scene_file, "--output", tmp_path / "y.png", "--frames", 2, "--rebuild-device")
    assert r.returncode != 0 and "--rebuild-device needs" in r.stderr and not os.path.exists(tmp_path / "y.png")
