"""Tree cost and rebuild on the MI355X (include/hpt.h, "tree cost" and "rebuild").  The device's cost is held to the bytes of
the host definition over the tree the device exports, on every scene of rebuild_cases.py and after every step of
refit_cases.py; a rebuilt handle is held to the builder's bytes for the records it holds, renders what it rendered before
under every way the path tracer walks the tree, and keeps everything else it held -- shown against a twin handle that did
not rebuild.  Every render is 48 x 48, 4 spp; one long-lived handle per case."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cost_oracle as co
import guides_oracle
import pose_cases as pc
import ppm_oracle
import rebuild_cases as rb
import refit_cases as rc
import skin_cases as sc
from path_tracing_amd import scene_io as sio
from test_bvh_walk import COUNT_KEYS
from test_gpu_refit import TREE_KEYS, _apply, _params, _probe_rays, _same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "path_tracing_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")
MOTION_KEYS = ("albedo", "normal", "position", "coverage", "prev_position")
UPDATE_COUNTS = ("updates", "live_tris", "dead_tris")


def _cost_is_the_definition(hpt, scene, what):
    """The whole struct: the device's reduction against hpt_bvh_cost_host of the tree the device exports."""
    got, want = scene.tree_cost(), hpt.tree_cost_host(scene.export_bvh())
    co.same(what, got, want)
    assert got["bytes"] == want["bytes"], what
    return got


def _same_tree(what, got, want):
    for k in TREE_KEYS:
        _same("%s: exported %s" % (what, k), got[k], want[k])


def _pt(hpt, scene, cam, flags=0, budget=0):
    return scene.render_pt(cam, rb.W, rb.H, rb.DEPTH, rb.SPP, _params(hpt, flags, budget))


# ---- the cost on the device ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rb.HOST_NAMES)
def test_device_cost_equals_the_host_definition(hpt, name):
    """Before a render, twice in a row (the result buffer is zeroed by every call), and after a render."""
    L, sp, tr = rb.host_scene(name)
    with hpt.Scene(L, sp, tr) as scene:
        first = _cost_is_the_definition(hpt, scene, name + ", before a render")
        co.same(name + ", against the builder's tree on the host", first, hpt.tree_cost_host(hpt.export_bvh_host(L, sp, tr)))
        co.same(name + ", twice in a row", scene.tree_cost(), first)
        scene.render_pt(rc.camera(), rb.W, rb.H, rb.DEPTH, 1, hpt.make_params(seed=rb.SEED))
        co.same(name + ", after a render", _cost_is_the_definition(hpt, scene, name + ", after a render"), first)
        if name.startswith("nodes-"):
            assert first["num_nodes"] == int(name[6:])


def test_device_cost_where_the_stride_loop_takes_a_second_trip(hpt):
    L, sp, tr = rb.big()
    with hpt.Scene(L, sp, tr) as scene:
        got = _cost_is_the_definition(hpt, scene, "grid-stride")
        assert got["num_nodes"] > 256 * 256 and got["leaf_slots"] == len(tr) == sc.N_STRIDE
        co.same("grid-stride, twice in a row", scene.tree_cost(), got)


@pytest.mark.parametrize("name", rc.NAMES)
def test_device_cost_after_every_step_of_the_refit_cases(hpt, name):
    d = rc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        for step in range(len(d.steps)):
            _apply(scene, name, step)
            got = _cost_is_the_definition(hpt, scene, "%s step %d" % (name, step))
            co.same("%s step %d, against the host's refit" % (name, step), got, hpt.tree_cost_host(rc.tree(hpt, name, step)))


# ---- rebuild -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rb.STATE_NAMES)
def test_rebuild_from_a_starting_state(hpt, oracle_mod, name):
    st = rb.state(name)
    L, sp, _ = st.base
    with hpt.Scene(*st.base) as scene:
        rb.enter(scene, st)
        T = scene.read_triangles()
        assert int(rc.dead(T).sum()) == rb.N_DEAD[name]
        before_img, before_cost, before_tree = _pt(hpt, scene, st.camera), scene.tree_cost(), scene.export_bvh()
        before_stats, info0 = scene.stats(), scene.update_info()
        assert scene.rebuild_info()["rebuilds"] == 0
        scene.rebuild()
        # the builder's tree for the records the handle holds, byte for byte
        want = hpt.export_bvh_host(L, sp, T)
        dev = scene.export_bvh()
        _same_tree(name + " rebuilt", dev, want)
        _same(name + ": the records are untouched", scene.read_triangles(), T)
        stats, ri = scene.stats(), scene.rebuild_info()
        assert (stats["bvh_nodes"], stats["bvh_depth"]) == (dev["num_nodes"], dev["bvh_depth"]) == (ri["nodes_after"], ri["depth_after"])
        assert (ri["nodes_before"], ri["depth_before"]) == (before_tree["num_nodes"], before_tree["bvh_depth"]) == (before_stats["bvh_nodes"], before_stats["bvh_depth"])
        assert ri["rebuilds"] == 1 and ri["ms_build"] > 0 and ri["ms_upload"] > 0 and ri["ms_download"] >= 0
        assert (stats["n_tris"], stats["n_materials"]) == (before_stats["n_tris"], before_stats["n_materials"])
        assert scene.update_info() == info0
        # the image does not depend on the tree: its own bytes from before, and the scan's, however the tree is walked
        scan, _ = oracle_mod.pt_render(L, sp, T, st.camera, rb.W, rb.H, rb.DEPTH, rb.SPP, seed=rb.SEED)
        _same(name + ": the image before the rebuild against the scan", before_img, scan)
        for what, flags, budget in (("default", 0, 0), ("budget 1", 0, 1), ("budget 63", 0, 63), ("brute force", hpt.FLAG_BRUTE_FORCE, 0),
                                    ("counting", hpt.FLAG_COUNT_WORK, 0)):
            _same("%s rebuilt: render_pt, %s" % (name, what), _pt(hpt, scene, st.camera, flags, budget), before_img)
        counted = scene.stats()
        walk, so = oracle_mod.pt_render(L, sp, T, st.camera, rb.W, rb.H, rb.DEPTH, rb.SPP, seed=rb.SEED, bvh=dev)
        assert np.array_equal(walk, scan), name
        assert {k: int(counted[k]) for k in COUNT_KEYS} == {k: int(so[k]) for k in COUNT_KEYS}, name
        # the probes walk the float nodes
        o, d, p2 = _probe_rays(T, 7)
        t, prim = scene.trace_closest(o, d)
        tb, primb = scene.trace_closest(o, d, brute_force=True)
        _same(name + ": trace_closest prim against brute force", prim, primb)
        _same(name + ": trace_closest t against brute force", t, tb)
        _same(name + ": trace_visibility against brute force", scene.trace_visibility(o, p2), scene.trace_visibility(o, p2, brute_force=True))
        # the cost: the definition's, a fresh handle's, and for scramble below the refitted tree's
        cost = _cost_is_the_definition(hpt, scene, name + " rebuilt")
        with hpt.Scene(L, sp, T) as fresh:
            co.same(name + ": cost against a fresh handle of the same records", cost, fresh.tree_cost())
            _same_tree(name + ": a fresh handle", fresh.export_bvh(), want)
        print("%s: sah %.3f -> %.3f, nodes %d -> %d, depth %d -> %d" % (name, before_cost["sah"], cost["sah"], ri["nodes_before"], ri["nodes_after"],
                                                                         ri["depth_before"], ri["depth_after"]))
        if name == "scramble":
            assert cost["sah"] < before_cost["sah"]


def test_two_rebuilds_in_a_row_and_a_scene_of_no_triangles(hpt):
    st = rb.state("scramble")
    with hpt.Scene(*st.base) as scene:
        rb.enter(scene, st)
        scene.rebuild()
        tree, img, cost, ri, stats = scene.export_bvh(), _pt(hpt, scene, st.camera), scene.tree_cost(), scene.rebuild_info(), scene.stats()
        scene.rebuild()
        _same_tree("the second rebuild", scene.export_bvh(), tree)
        _same("the second rebuild: render_pt", _pt(hpt, scene, st.camera), img)
        co.same("the second rebuild: cost", scene.tree_cost(), cost)
        ri2 = scene.rebuild_info()
        assert ri2["rebuilds"] == 2 and (ri2["nodes_before"], ri2["depth_before"]) == (ri["nodes_after"], ri["depth_after"]) == (ri2["nodes_after"], ri2["depth_after"])
        assert all(scene.stats()[k] == stats[k] for k in ("bvh_nodes", "bvh_depth", "n_tris", "n_materials"))
    L, sp, tr = rb.host_scene("tiny-0")
    with hpt.Scene(L, sp, tr) as scene:
        scene.rebuild()
        assert scene.rebuild_info()["rebuilds"] == 1
        _same_tree("no triangles", scene.export_bvh(), hpt.export_bvh_host(L, sp, tr))
        _cost_is_the_definition(hpt, scene, "no triangles, rebuilt")


# ---- what a rebuild leaves alone: a twin handle that does not rebuild -------------------------------------------------------

def _motion_guides(hpt, scene, cam):
    return scene.render_guides(cam, rb.W, rb.H, rb.SPP, hpt.make_params(seed=7), prev_position=True)


def _twins_agree(hpt, a, b, cam, what):
    assert a.has_motion() == b.has_motion(), what
    ia, ib = a.update_info(), b.update_info()
    assert {k: ia[k] for k in UPDATE_COUNTS} == {k: ib[k] for k in UPDATE_COUNTS}, what
    ga, gb = _motion_guides(hpt, a, cam), _motion_guides(hpt, b, cam)
    for k in MOTION_KEYS:
        _same("%s: motion guide %s" % (what, k), ga[k].view(np.uint32), gb[k].view(np.uint32))
    _same(what + ": render_pt", _pt(hpt, a, cam), _pt(hpt, b, cam))


def _pose_calls():
    d = pc.data("turn")
    return (d.L, d.sp, d.tr), [("set_parts", (d.steps[0][1], d.steps[0][2]))] + [("pose", (s[1],)) for s in d.steps[1:]]


def _skin_calls():
    d = sc.data("bend")
    return (d.L, d.sp, d.tr), [("set_skin", d.steps[0][1:])] + [("skin", (s[1],)) for s in d.steps[1:]]


def _triangle_calls():
    d = rc.data("turn")
    return (d.L, d.sp, d.tr), [("update_triangles", (rc.records("turn", s)[2],)) for s in range(len(d.steps))]


@pytest.mark.parametrize("kind", ["pose", "skin", "update_triangles"])
def test_a_rebuild_in_the_middle_of_a_sequence(hpt, kind):
    """Twins take the same calls; one rebuilds after the second geometry step, with a previous geometry kept one step back.
    Afterwards: the same motion flag, update counts and five motion guides (the previous geometry is untouched), the same
    update_info as before the rebuild, and the next step refits the NEW topology: the tree of
    hpt_bvh_refit_host(records at the rebuild, new records), with the twin's image."""
    base, calls = dict(pose=_pose_calls, skin=_skin_calls, update_triangles=_triangle_calls)[kind]()
    cam = rc.camera()
    setup = [c for c in calls if c[0].startswith("set_")]
    moves = [c for c in calls if not c[0].startswith("set_")]
    assert len(moves) >= 3
    with hpt.Scene(*base) as a, hpt.Scene(*base) as b:
        for s in (a, b):
            rb.enter(s, rb.State(base, setup + moves[:1], cam, None))
            s.keep_previous()                                        # G' is the first step's geometry ...
            rb.enter(s, rb.State(base, moves[1:2], cam, None))       # ... and G the second's
        info = a.update_info()
        at_rebuild = a.read_triangles()
        a.rebuild()
        assert a.update_info() == info and a.rebuild_info()["rebuilds"] == 1 and b.rebuild_info()["rebuilds"] == 0
        _same_tree(kind + ": rebuilt", a.export_bvh(), hpt.export_bvh_host(base[0], base[1], at_rebuild))
        _twins_agree(hpt, a, b, cam, kind + " after the rebuild")
        for s in (a, b):
            rb.enter(s, rb.State(base, moves[2:3], cam, None))
        moved = b.read_triangles()
        _same(kind + ": the records after the next step", a.read_triangles(), moved)
        assert moved.tobytes() != at_rebuild.tobytes()
        _same_tree(kind + ": the next step refits the new topology", a.export_bvh(), hpt.refit_bvh_host(base[0], base[1], at_rebuild, moved))
        _twins_agree(hpt, a, b, cam, kind + " after the next step")
        _cost_is_the_definition(hpt, a, kind + " after the next step")


def test_bdpt_groups_ppm_bounds_and_guides_across_a_rebuild(hpt, oracle_mod, tmp_path):
    """skin_cases' bend: groups set and every lazy structure built (a BDPT render, a photon-mapping render with null bounds)
    before the rebuild; afterwards the three renders are the oracles' bytes, as they were."""
    name, step = "bend", 2
    d = sc.data(name)
    L, sp, tr = sc.records(name, step)
    plib, glib = ppm_oracle.build(tmp_path), guides_oracle.build(tmp_path)
    kw = dict(eye_depth=4, light_depth=4, spp=1, spl=256, radius=0.07, seed=5)
    cam = sc.camera(name)
    bcam = sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, sc.W, sc.H, tan_in_float=True)

    def renders(scene):
        return (scene.render_bdpt(bcam, sc.W, sc.H, 4, 4, sc.SPP, 8, hpt.make_params(seed=3)),
                scene.render_ppm(cam, sc.W, sc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"], hpt.make_params(seed=kw["seed"])),
                scene.render_guides(cam, sc.W, sc.H, sc.SPP, hpt.make_params(seed=5)))

    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        scene.set_groups(*d.order)
        scene.set_skin(*d.steps[0][1:])
        for s in range(1, step + 1):
            scene.skin(d.steps[s][1])
        before = renders(scene)
        scene.rebuild()
        after = renders(scene)
        want_bdpt = oracle_mod.bdpt_render(L, sp, tr, d.order, d.eye, d.look, sio.CORNELL_UP, 50.0, sc.W, sc.H, 4, 4, sc.SPP, 8, seed=3)[0]
        want_ppm = ppm_oracle.render(plib, L, sp, tr, cam, sc.W, sc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"], seed=kw["seed"])[0]
        want_guides, _ = guides_oracle.render(glib, L, sp, tr, cam, sc.W, sc.H, sc.SPP, seed=5)
        for what, imgs in (("before", before), ("after", after)):
            _same("bend, %s the rebuild: BDPT with groups" % what, imgs[0], want_bdpt)
            _same("bend, %s the rebuild: PPM with null bounds" % what, imgs[1], want_ppm)
            for k in ("albedo", "normal", "position", "coverage"):
                _same("bend, %s the rebuild: guide %s" % (what, k), imgs[2][k], want_guides[k])


def test_an_sppm_state_continues_across_a_rebuild(hpt):
    st = rb.state("scramble")
    kw = dict(eye_depth=4, light_depth=4, spl=256, radius=0.07, alpha=0.7)
    with hpt.Scene(*st.base) as a, hpt.Scene(*st.base) as b:
        states = []
        for s in (a, b):
            rb.enter(s, st)
            states.append(s.sppm(st.camera, rb.W, rb.H, params=hpt.make_params(seed=5), **kw))
        try:
            for p in states:
                p.render(2)
            a.rebuild()
            ia, ib = states[0].render(2), states[1].render(2)
            _same("SPPM after the rebuild, passes 3 and 4", ia, ib)
            sa, sb = states[0].state(), states[1].state()
            assert sa["passes"] == sb["passes"] == 4
            _same("SPPM radius", sa["radius2"], sb["radius2"])
            _same("SPPM photons", sa["photons"], sb["photons"])
        finally:
            for p in states:
                p.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_as_it_was(hpt):
    st = rb.state("dead-20")
    lib = hpt.load_library()
    out = hpt.TreeCost()
    with hpt.Scene(*st.base) as scene:
        rb.enter(scene, st)
        img, tree, cost = _pt(hpt, scene, st.camera), scene.export_bvh(), scene.tree_cost()
        assert lib.hpt_scene_tree_cost(scene._h, None) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_tree_cost(None, C.byref(out)) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_rebuild(None) == 1 and b"null scene" in lib.hpt_last_error()
        assert lib.hpt_scene_get_rebuild_info(scene._h, None) == 1 and b"null" in lib.hpt_last_error()
        if hpt.device_count() >= 2:
            import torch
            torch.cuda.set_device(1)
            try:
                for call in (scene.tree_cost, scene.rebuild):
                    with pytest.raises(hpt.HptError) as e:
                        call()
                    assert str(e.value).startswith("hpt error 1:") and "another device" in str(e.value)
            finally:
                torch.cuda.set_device(0)
        assert scene.rebuild_info()["rebuilds"] == 0
        _same_tree("after the refusals", scene.export_bvh(), tree)
        _same("after the refusals: render_pt", _pt(hpt, scene, st.camera), img)
        co.same("after the refusals: cost", scene.tree_cost(), cost)


# ---- CLI --------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(CSRC, "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_rebuild_above_rebuilds_and_keeps_the_image(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    obj = str(tmp_path / "mesh.obj")
    sio.write_obj(obj, sio._tris_from(sio.tessellated_sphere((-0.15, 0.25, 0.0), 0.15, 12, 12), np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), np.float32), (264, 1))))
    base = ["--mode", "pt", "--input", scene_file, "--obj", obj, "--seed", 13, "--width", 64, "--height", 48, "--frame-spp", 2, "--guide-spp", 3,
            "--frames", 4, "--twist-device", 20, "--reproject"]
    plain = _cli(*base, "--output", tmp_path / "plain.png")
    assert plain.returncode == 0 and "[Success] Image saved!" in plain.stdout and "[Rebuild]" not in plain.stdout, plain.stdout + plain.stderr
    # a small mesh twisted in a large room moves the tree's cost by a quarter of a percent (host definition: x 1.0025 after 20
    # degrees), so the ratio is set far below that; any ratio above 1 is a valid one
    run = _cli(*base, "--output", tmp_path / "rebuilt.png", "--rebuild-above", 1.0005)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    lines = re.findall(r"^\[Rebuild\] frame (\d+) sah (\S+) -> (\S+) (\S+) ms$", run.stdout, flags=re.M)
    assert len(lines) >= 1, run.stdout
    for frame, before, after, ms in lines:
        assert 1 <= int(frame) <= 3 and float(before) > 0.0 and float(after) > 0.0 and float(ms) > 0.0
    frames = lambda text: re.findall(r"^\[Frame \d+\].*$", text, flags=re.M)
    assert frames(run.stdout) == frames(plain.stdout) and len(frames(run.stdout)) == 4            # rms and kept share: the history follows across it
    with open(tmp_path / "plain.png", "rb") as f, open(tmp_path / "rebuilt.png", "rb") as g:
        assert f.read() == g.read()
    for bad in ("1", "0.5", "nan", "-3"):
        out = tmp_path / ("bad%s.png" % bad)
        r = _cli(*base, "--output", out, "--rebuild-above", bad)
        assert r.returncode != 0 and "--rebuild-above" in r.stderr and not os.path.exists(out), bad
    r = _cli("--mode", "pt", "--input", scene_file, "--output", tmp_path / "y.png", "--frames", 2, "--rebuild-above", 2)
    assert r.returncode != 0 and "--rebuild-above needs" in r.stderr and not os.path.exists(tmp_path / "y.png")
