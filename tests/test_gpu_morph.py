"""Morph targets on the MI355X (include/hpt.h, "morph targets"): every case of morph_cases.py on ONE long-lived handle, step
after step through Scene.set_morphs, Scene.morph, Scene.set_parts, Scene.pose, Scene.set_skin, Scene.skin,
Scene.update_triangles and Scene.update_vertices_device.  After every step the exported tree is held to the bytes of
hpt_bvh_refit_host of the records morph_oracle (with pose_oracle and skin_oracle) expects, Scene.read_triangles to
hpt_morph_host's records composed with hpt_pose_host / hpt_skin_host, and the path tracer to the oracle's image of them.
A morph is held to a twin handle given the same records through update_triangles; a scene with morphs at zero weights to a
twin without morphs, posed and skinned beside it; the lazy host-record paths (the bidirectional scene, photon mapping's own
bounds) and the guides to their oracles after morphs; the per-frame chain of "motion" runs on morphs; a rebuild between two
morphs is held to a twin that did not rebuild; the refusals leave the handle as it was; pt_cli --morph-device runs.
tests/test_morph_cpu.py keeps every step's image distinct from the one before and `order` and `contract` sensitive to the
order of the sum and to contraction."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guides_oracle
import morph_cases as mc
import morph_oracle as mo
import motion_oracle
import pose_cases as pc
import pose_oracle as po
import ppm_oracle
import refit_cases as rc
import skin_cases as sc
from path_tracing_amd import scene_io as sio

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "path_tracing_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")
TREE_KEYS = ("num_nodes", "num_tris", "bvh_depth", "num_rounds", "qorigin", "qscale", "qnodes", "tris")
GUIDE_KEYS = ("albedo", "normal", "position", "coverage")
U32 = np.uint32


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


def _same(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        if got.dtype.names:
            got, want = po.verts_of(got), po.verts_of(want)
        bits = "u%d" % got.dtype.itemsize
        diff = np.argwhere(got.view(bits) != want.view(bits))
        at = tuple(int(v) for v in diff[0]) if len(diff) else ()
        pytest.fail("%s differs in %d of %d values, first at %s" % (what, len(diff), got.size, at))


def _same_tree(what, got, want):
    for k in TREE_KEYS:
        _same("%s: exported %s" % (what, k), got[k], want[k])


def _pt(hpt, scene, name, flags=0):
    return scene.render_pt(mc.camera(name), mc.W, mc.H, mc.DEPTH, mc.SPP, hpt.make_params(seed=mc.SEED, flags=flags))


def _do(torch, scene, s):
    if s[0] == "morphs":
        scene.set_morphs(s[1], s[2], s[3])
    elif s[0] == "morph":
        scene.morph(s[1])
    elif s[0] == "set":
        scene.set_skin(s[1], s[2], s[3])
    elif s[0] == "skin":
        scene.skin(s[1])
    elif s[0] == "parts":
        scene.set_parts(s[1], s[2])
    elif s[0] == "pose":
        scene.pose(s[1])
    elif s[0] == "tris":
        scene.update_triangles(s[1])
    else:
        scene.update_vertices_device(torch.from_numpy(po.verts_of(s[1])).cuda())


def _apply(torch, scene, name, step):
    _do(torch, scene, mc.data(name).steps[step])


# ---- every case on one handle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mc.NAMES)
def test_case_on_one_handle(hpt, torch, oracle_mod, name):
    """Tree bytes, read_triangles against the host definitions, the PT renders and the update counts after every step."""
    d = mc.data(name)
    renders = (("default", 0),) if d.walk else (("default", 0), ("brute force", hpt.FLAG_BRUTE_FORCE))
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _same(name + ": base render", _pt(hpt, scene, name), mc.scan(oracle_mod, name, -1, hpt)[0])       # workspaces exist before the first update
        updates = 0
        for step in range(len(d.steps)):
            where = "%s step %d" % (name, step)
            assert not scene.has_motion() or updates > 0, where
            _apply(torch, scene, name, step)
            st = mc.expected(name)[step]
            _same_tree(where, scene.export_bvh(), mc.tree(hpt, name, step))
            info = scene.update_info()
            if mc.is_geometry_step(name, step):
                updates += 1
                n_dead = int(rc.dead(st.tr).sum())
                assert (info["dead_tris"], info["live_tris"]) == (n_dead, len(st.tr) - n_dead), where
                if (name, step) in mc.N_DEAD:
                    assert n_dead == mc.N_DEAD[(name, step)]
                if d.steps[step][0] != "tris":
                    assert info["ms_pack"] == 0.0 and info["ms_upload"] > 0 and info["ms_refit"] > 0, where
            assert info["updates"] == updates, where
            scan = mc.scan(oracle_mod, name, step, hpt)[0]
            for what, flags in renders:
                _same("%s: render_pt, %s" % (where, what), _pt(hpt, scene, name, flags), scan)
            got = scene.read_triangles()
            _same(where + ": read_triangles", got, st.tr)
            _same(where + ": read_triangles against the host definitions", got, mc.host_chain(hpt, st))


def test_zero_weights_preserve_minus_zero_and_the_nan_payload_on_the_device(hpt, torch):
    d = mc.data("zero")
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        for step in range(3):
            _apply(torch, scene, "zero", step)
            got = scene.read_triangles()
            assert got.tobytes() == d.tr.tobytes(), step
        bits = po.verts_of(got).view(U32)
        assert bits[0, 1, 0] == 0x80000000 and bits[11, 2, 1] == 0x7FC12345
        _same_tree("zero step 2 against the builder's tree", scene.export_bvh(), hpt.export_bvh_host(d.L, d.sp, d.tr))
        _apply(torch, scene, "zero", 3)                                                     # the sphere bulges, the walls are kept
        bits = po.verts_of(scene.read_triangles()).view(U32)
        assert bits[0, 1, 0] == 0x80000000 and bits[11, 2, 1] == 0x7FC12345
        assert np.array_equal(bits[:mc.NWALL], po.verts_of(d.tr).view(U32)[:mc.NWALL])


# ---- twins ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["contract", "die-and-return", "with-skin"])
def test_a_morph_leaves_the_tree_and_image_of_a_twin_given_the_same_records(hpt, torch, name):
    d = mc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as morphed, hpt.Scene(d.L, d.sp, d.tr) as twin:
        for step in range(len(d.steps)):
            _apply(torch, morphed, name, step)
            if not mc.is_geometry_step(name, step):
                continue
            twin.update_triangles(mc.host_chain(hpt, mc.expected(name)[step]))
            where = "%s step %d against the twin" % (name, step)
            _same_tree(where, morphed.export_bvh(), twin.export_bvh())
            _same(where + ": render_pt", _pt(hpt, morphed, name), _pt(hpt, twin, name))
            a, b = morphed.update_info(), twin.update_info()
            assert (a["updates"], a["live_tris"], a["dead_tris"]) == (b["updates"], b["live_tris"], b["dead_tris"]), where


def test_a_scene_with_morphs_at_zero_weights_poses_and_skins_like_one_without(hpt, torch):
    """Parts and then a skin on two handles, one of which also holds targets whose weights stay zero (and once are given as
    zeros of both signs): the same trees and records throughout."""
    d = mc.data("swap")
    targets = d.steps[0][1:]
    bone, weight = sc.height_weights(d.tr)
    turn = lambda deg: pc.table(po.IDENTITY, pc.affine(pc.tilted(deg), mc.BEND_C))
    plain_steps = [("parts", pc.two_parts(len(d.tr)), 2), ("pose", turn(30.0)), ("pose", turn(65.0)), ("set", bone, weight, 2),
                   ("skin", sc.twist(40.0, mc.BEND_C)), ("skin", sc.twist(-80.0, mc.BEND_C))]
    neg0 = np.array([0x80000000], U32).view(np.float32)[0]
    with hpt.Scene(d.L, d.sp, d.tr) as with_morphs, hpt.Scene(d.L, d.sp, d.tr) as plain:
        with_morphs.set_morphs(*targets)
        for i, s in enumerate(plain_steps):
            _do(torch, with_morphs, s)
            _do(torch, plain, s)
            if i == 2:
                with_morphs.morph(mc.w(neg0, 0.0))                  # all inactive: M = R, the deformer's last table over it
            where = "zero-weight morphs beside none, step %d" % i
            _same_tree(where, with_morphs.export_bvh(), plain.export_bvh())
            _same(where + ": read_triangles", with_morphs.read_triangles(), plain.read_triangles())


def test_a_rebuild_between_two_morphs_keeps_targets_weights_and_the_morphed_rest_pose(hpt, torch, oracle_mod):
    name = "with-parts"
    d = mc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as rebuilt, hpt.Scene(d.L, d.sp, d.tr) as twin:
        for step in range(3):                                      # morphs, parts, a morph
            _apply(torch, rebuilt, name, step)
            _apply(torch, twin, name, step)
        rebuilt.rebuild()
        at_rebuild = mc.records(name, 2)[2]
        _same("rebuild: read_triangles", rebuilt.read_triangles(), at_rebuild)
        _same_tree("rebuild", rebuilt.export_bvh(), hpt.export_bvh_host(d.L, d.sp, at_rebuild))
        for step in range(3, len(d.steps)):                        # a pose over the M the rebuild kept, a morph, a pose
            _apply(torch, rebuilt, name, step)
            _apply(torch, twin, name, step)
            where = "%s step %d after a rebuild" % (name, step)
            tr = mc.records(name, step)[2]
            _same(where + ": read_triangles", rebuilt.read_triangles(), twin.read_triangles())
            _same(where + ": read_triangles", rebuilt.read_triangles(), tr)
            _same_tree(where, rebuilt.export_bvh(), hpt.refit_bvh_host(d.L, d.sp, at_rebuild, tr))
            scan = mc.scan(oracle_mod, name, step)[0]
            _same(where + ": render_pt", _pt(hpt, rebuilt, name), scan)
            _same(where + ": render_pt of the twin", _pt(hpt, twin, name), scan)
        assert rebuilt.rebuild_info()["rebuilds"] == 1 and rebuilt.update_info()["updates"] == twin.update_info()["updates"] == 4


# ---- the other integrators: the lazy host records -------------------------------------------------------------------------

def _bdpt(hpt, scene, d):
    cam = sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, mc.W, mc.H, tan_in_float=True)
    return scene.render_bdpt(cam, mc.W, mc.H, 4, 4, mc.SPP, 8, hpt.make_params(seed=3))


def _bdpt_oracle(oracle_mod, d, L, sp, tr):
    return oracle_mod.bdpt_render(L, sp, tr, d.order, d.eye, d.look, sio.CORNELL_UP, 50.0, mc.W, mc.H, 4, 4, mc.SPP, 8, seed=3)[0]


PPM = dict(eye_depth=4, light_depth=4, spp=1, spl=256, radius=0.07, seed=5)
# (name, step, photon mapping too): photon mapping where every vertex is finite, as in the pose and skin suites
OTHERS = [("with-skin", 2, True), ("with-skin", 3, True), ("die-and-return", 2, False), ("die-and-return", 3, True)]


@pytest.mark.parametrize("name", ["with-skin", "die-and-return"])
def test_bdpt_ppm_and_guides_after_morphs(hpt, torch, oracle_mod, tmp_path, name):
    """Groups set and the bidirectional scene built before the first step; then, after morphs that nobody read back, BDPT
    and photon mapping with null bounds -- both built from the handle's host records, which a morph leaves behind the
    device's vertices -- and the guides."""
    d = mc.data(name)
    plib, glib = ppm_oracle.build(tmp_path), guides_oracle.build(tmp_path)
    kw = PPM
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        scene.set_groups(*d.order)
        _same(name + ": BDPT of the base scene", _bdpt(hpt, scene, d), _bdpt_oracle(oracle_mod, d, d.L, d.sp, d.tr))
        done = -1
        for case, step, with_ppm in OTHERS:
            if case != name:
                continue
            while done < step:
                done += 1
                _apply(torch, scene, name, done)
            where = "%s step %d" % (name, step)
            L, sp, tr = mc.records(name, step)
            got = scene.render_guides(mc.camera(name), mc.W, mc.H, mc.SPP, hpt.make_params(seed=5))
            want, _ = guides_oracle.render(glib, L, sp, tr, mc.camera(name), mc.W, mc.H, mc.SPP, seed=5)
            for k in GUIDE_KEYS:
                _same("%s: guide %s" % (where, k), got[k], want[k])
            _same(where + ": BDPT", _bdpt(hpt, scene, d), _bdpt_oracle(oracle_mod, d, L, sp, tr))
            if with_ppm:
                got = scene.render_ppm(mc.camera(name), mc.W, mc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"],
                                       hpt.make_params(seed=kw["seed"]))
                want = ppm_oracle.render(plib, L, sp, tr, mc.camera(name), mc.W, mc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"],
                                         kw["radius"], seed=kw["seed"])[0]
                _same(where + ": PPM with null bounds", got, want)


# ---- motion ------------------------------------------------------------------------------------------------------------

def test_the_per_frame_chain_of_motion_on_morphs(hpt, tmp_path):
    """pose_cases' sphere bulged further every frame: morph, render_guides(prev_position=True), keep_previous.
    prev_position is motion_oracle's bytes, and on the pixels whose samples all end on the walls -- no target names them --
    it equals position bit for bit."""
    L, sp, tr0 = pc.base()
    targets = mc.two_shapes(tr0, centre=rc.SPHERE_C)
    mlib, glib = motion_oracle.build(tmp_path), guides_oracle.build(tmp_path)
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, mc.W, mc.H)
    walls_only, _ = guides_oracle.render(glib, L, sp, tr0[:mc.NWALL], cam, mc.W, mc.H, mc.SPP, seed=7)
    with hpt.Scene(L, sp, tr0) as scene:
        scene.set_morphs(*targets)
        assert not scene.has_motion()                              # set_morphs changes no geometry
        prev = tr0
        for frame, wts in enumerate((mc.w(0.0, 0.0), mc.w(0.2, 0.3), mc.w(0.4, 0.6), mc.w(0.6, -0.2))):
            scene.morph(wts)
            tr = mo.morph(tr0, *targets, wts)
            assert scene.has_motion()
            got = scene.render_guides(cam, mc.W, mc.H, mc.SPP, hpt.make_params(seed=7), prev_position=True)
            want, _ = motion_oracle.render(mlib, L, sp, tr, sp, prev, cam, mc.W, mc.H, mc.SPP, seed=7)
            for k in motion_oracle.KEYS:
                a, b = got[k], want[k]
                bad = (a.view(U32) != b.view(U32)) & ~(np.isnan(a) & np.isnan(b))
                assert not bad.any(), ("frame %d: guide %s" % (frame, k), int(bad.sum()))
            wall = (got["position"].view(U32) == walls_only["position"].view(U32)).all(axis=-1) & (got["coverage"] > 0)
            assert wall.mean() > 0.5
            assert np.array_equal(got["prev_position"].view(U32)[wall], got["position"].view(U32)[wall]), frame
            moved = (got["prev_position"].view(U32) != got["position"].view(U32)).any(axis=-1)
            if frame == 0:
                assert not moved.any()                             # every weight zero: keep, the same bits
            else:
                assert moved.mean() > 0.02, frame
            scene.keep_previous()
            assert not scene.has_motion()
            prev = tr


# ---- refusals -------------------------------------------------------------------------------------------------------------

def _refused(hpt, call, *words):
    with pytest.raises(hpt.HptError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith("hpt error 1:"), msg
    for word in words:
        assert word in msg, msg


def test_refused_calls_leave_the_handle_as_it_was(hpt, torch, oracle_mod):
    name = "with-parts"
    d = mc.data(name)
    n = len(d.tr)
    tb, ec, ed = d.steps[0][1:]
    good = d.steps[2][1]
    lib = hpt.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def edited(a, at, value):
        a = a.copy(); a[at] = value
        return a
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _refused(hpt, lambda: scene.morph(good), "before hpt_scene_set_morphs")
        scene.set_parts(None, 1)
        _refused(hpt, lambda: scene.morph(good), "before hpt_scene_set_morphs")        # parts are no morphs
        for step in range(4):                                      # morphs, parts, a morph, a pose
            _apply(torch, scene, name, step)
        want_img, want_tree, info = _pt(hpt, scene, name), scene.export_bvh(), scene.update_info()
        assert lib.hpt_scene_set_morphs(scene._h, vp(tb), vp(ec), vp(ed), len(ec), n - 1, 2) == 1 and b"count" in lib.hpt_last_error()
        _refused(hpt, lambda: scene.set_morphs(tb, ec, ed[:-1]), "three floats per entry")
        assert lib.hpt_scene_set_morphs(scene._h, vp(tb), vp(ec), vp(ed), len(ec), n, 0) == 1 and b"[1, 4096]" in lib.hpt_last_error()
        assert lib.hpt_scene_set_morphs(scene._h, vp(tb), vp(ec), vp(ed), len(ec), n, 4097) == 1 and b"[1, 4096]" in lib.hpt_last_error()
        assert lib.hpt_scene_set_morphs(scene._h, vp(tb), vp(ec), vp(ed), -1, n, 2) == 1 and b"negative morph entry count" in lib.hpt_last_error()
        _refused(hpt, lambda: scene.set_morphs(edited(tb, 0, 1), ec, ed), "target_begin[0] must be 0")
        _refused(hpt, lambda: scene.set_morphs(edited(tb, 1, len(ec) + 1), ec, ed), "target_begin decreases at target 1")
        _refused(hpt, lambda: scene.set_morphs(edited(tb, 2, len(ec) - 1), ec, ed), "must be the number of entries")
        _refused(hpt, lambda: scene.set_morphs(tb, edited(ec, 5, 3 * n), ed), "of target 0 (entry 5) is not one of the %d corners" % (3 * n))
        _refused(hpt, lambda: scene.set_morphs(tb, edited(ec, tb[1] + 4, -2), ed), "corner -2 of target 1 (entry %d)" % (tb[1] + 4))
        _refused(hpt, lambda: scene.set_morphs(tb, edited(ec, 7, ec[6]), ed), "target 0 are not strictly ascending", "entry 7")
        assert lib.hpt_scene_set_morphs(scene._h, None, vp(ec), vp(ed), len(ec), n, 2) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_set_morphs(scene._h, vp(tb), None, vp(ed), len(ec), n, 2) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_set_morphs(scene._h, vp(tb), vp(ec), None, len(ec), n, 2) == 1 and b"null" in lib.hpt_last_error()
        _refused(hpt, lambda: scene.morph(mc.w(1.0)), "keeps the number of targets", "2 targets, 1 weights")
        _refused(hpt, lambda: scene.morph(mc.w(1.0, 1.0, 1.0)), "keeps the number of targets")
        assert lib.hpt_scene_morph(scene._h, None, 2) == 1 and b"null weight array" in lib.hpt_last_error()
        if hpt.device_count() >= 2:
            torch.cuda.set_device(1)
            try:
                _refused(hpt, lambda: scene.morph(good), "another device")
                _refused(hpt, lambda: scene.set_morphs(tb, ec, ed), "another device")
            finally:
                torch.cuda.set_device(0)
        # ... the handle is as it was: the targets, the rest pose, M and the table too (the next steps give the expected scenes)
        assert scene.update_info() == info
        _same("after the refusals: render_pt", _pt(hpt, scene, name), want_img)
        _same_tree("after the refusals", scene.export_bvh(), want_tree)
        for step in (4, 5):
            _apply(torch, scene, name, step)
            _same_tree("after the refusals, step %d" % step, scene.export_bvh(), mc.tree(hpt, name, step))
            _same("after the refusals, step %d: render_pt" % step, _pt(hpt, scene, name), mc.scan(oracle_mod, name, step)[0])


def test_a_scene_of_no_triangles_takes_every_call_with_zero_entries(hpt, torch):
    d = mc.data("with-parts")
    empty = d.tr[:0]
    with hpt.Scene(d.L, d.sp, empty) as scene:
        scene.set_morphs(*mc.targets(mc.EMPTY))
        scene.morph(mc.w(1.0))
        scene.set_parts(None, 1)
        scene.set_morphs(*mc.targets(*([mc.EMPTY] * 4096)))
        scene.morph(np.ones(4096, np.float32))
        scene.pose(pc.identity(1))
        assert len(scene.read_triangles()) == 0
        assert len(hpt.morph_host(empty, *mc.targets(mc.EMPTY, mc.EMPTY), mc.w(1.0, 2.0))) == 0
        assert scene.update_info()["updates"] == 3
        _same_tree("no triangles", scene.export_bvh(), hpt.export_bvh_host(d.L, d.sp, empty))


# ---- CLI ------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(CSRC, "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_morph_device_alone_and_with_twist_device_reproject(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    obj = str(tmp_path / "mesh.obj")
    sio.write_obj(obj, sio._tris_from(sio.tessellated_sphere((-0.15, 0.25, 0.0), 0.15, 12, 12), np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), np.float32), (264, 1))))
    base = ["--mode", "pt", "--input", scene_file, "--obj", obj, "--seed", 13, "--width", 64, "--height", 48, "--frame-spp", 2, "--guide-spp", 3]
    run = _cli(*base, "--output", tmp_path / "alone.png", "--frames", 3, "--morph-device", 0.8)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    rms = re.findall(r"^\[Frame \d+\] rms (\S+)", run.stdout, flags=re.M)
    assert len(rms) == 3, run.stdout
    still = _cli(*base, "--output", tmp_path / "still.png", "--frames", 3, "--morph-device", 0.0)
    assert still.returncode == 0, still.stdout + still.stderr
    assert open(tmp_path / "alone.png", "rb").read() != open(tmp_path / "still.png", "rb").read()      # the morph moved the mesh
    run = _cli(*base, "--output", tmp_path / "both.png", "--frames", 3, "--morph-device", 0.8, "--twist-device", 5, "--reproject")
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    kept = [float(v) for v in re.findall(r"^\[Frame \d+\] rms \S+ kept (\S+) %$", run.stdout, flags=re.M)]
    assert len(kept) == 3 and kept[0] == 0.0 and all(v > 0.0 for v in kept[1:]), run.stdout
    run = _cli(*base, "--output", tmp_path / "spin.png", "--frames", 2, "--morph-device", 0.5, "--spin-device", 10)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    run = _cli(*base, "--output", tmp_path / "x.png", "--frames", 3, "--morph-device", 0.5, "--spin", 5)
    assert run.returncode != 0 and "exclude each other" in run.stderr
    assert not os.path.exists(tmp_path / "x.png")
    run = _cli("--mode", "pt", "--input", scene_file, "--output", tmp_path / "y.png", "--morph-device", 0.5, "--frames", 2)
    assert run.returncode != 0 and "--morph-device needs --frames and --obj" in run.stderr
    assert not os.path.exists(tmp_path / "y.png")
