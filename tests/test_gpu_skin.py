"""Skinning on the MI355X (include/hpt.h, "skinning"): every case of skin_cases.py on ONE long-lived handle, step after
step through Scene.set_skin, Scene.skin, Scene.set_parts, Scene.pose, Scene.update_triangles and
Scene.update_vertices_device.  After every step the exported tree is held to the bytes of hpt_bvh_refit_host of the records
skin_oracle expects, Scene.read_triangles to hpt_skin_host's records, and the path tracer to the oracle's image of them.  A
one-hot skin is held to a twin handle that is posed; keep to -0 and the NaN payload; the lazy host-record paths (the
bidirectional scene, photon mapping's own bounds) and the guides to their oracles after skins; the per-frame chain of
"motion" runs on skins; the refusals leave the handle as it was; pt_cli --twist-device runs.  tests/test_skin_cpu.py keeps
every step's image distinct from the one before and `bend` sensitive to contraction."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guides_oracle
import motion_oracle
import pose_cases as pc
import pose_oracle as po
import ppm_oracle
import refit_cases as rc
import skin_cases as sc
import skin_oracle as so
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


def _pt(hpt, scene, name, flags=0):
    return scene.render_pt(sc.camera(name), sc.W, sc.H, sc.DEPTH, sc.SPP, hpt.make_params(seed=sc.SEED, flags=flags))


def _apply(torch, scene, name, step):
    s = sc.data(name).steps[step]
    if s[0] == "set":
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


def _check_tree(hpt, scene, name, step, want=None):
    dev, host = scene.export_bvh(), want or sc.tree(hpt, name, step)
    for k in TREE_KEYS:
        _same("%s step %d: exported %s" % (name, step, k), dev[k], host[k])


# ---- every case on one handle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.NAMES)
def test_case_on_one_handle(hpt, torch, oracle_mod, name):
    """Tree bytes, read_triangles against hpt_skin_host, the PT renders and the update counts after every step of the case."""
    d = sc.data(name)
    renders = (("default", 0),) if d.walk else (("default", 0), ("brute force", hpt.FLAG_BRUTE_FORCE))
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _same(name + ": base render", _pt(hpt, scene, name), sc.scan(oracle_mod, name, -1, hpt)[0])       # workspaces exist before the first update
        updates = 0
        for step in range(len(d.steps)):
            where = "%s step %d" % (name, step)
            assert not scene.has_motion() or updates > 0, where
            _apply(torch, scene, name, step)
            tr, rest, deformer = sc.expected(name)[step]
            _check_tree(hpt, scene, name, step)
            info = scene.update_info()
            if sc.is_geometry_step(name, step):
                updates += 1
                n_dead = int(rc.dead(tr).sum())
                assert (info["dead_tris"], info["live_tris"]) == (n_dead, len(tr) - n_dead), where
                if (name, step) in sc.N_DEAD:
                    assert n_dead == sc.N_DEAD[(name, step)]
                if d.steps[step][0] != "tris":
                    assert info["ms_pack"] == 0.0 and info["ms_upload"] > 0 and info["ms_refit"] > 0, where
            assert info["updates"] == updates, where
            scan = sc.scan(oracle_mod, name, step, hpt)[0]
            for what, flags in renders:
                _same("%s: render_pt, %s" % (where, what), _pt(hpt, scene, name, flags), scan)
            got = scene.read_triangles()
            _same(where + ": read_triangles", got, tr)
            if d.steps[step][0] == "skin":
                _same(where + ": read_triangles against hpt_skin_host", got, hpt.skin_host(rest, deformer[1], deformer[2], d.steps[step][1]))


def test_a_rigid_skin_leaves_the_tree_and_records_of_a_posed_twin(hpt, torch):
    d, p = sc.data("rigid"), pc.data("turn")
    with hpt.Scene(d.L, d.sp, d.tr) as skinned, hpt.Scene(p.L, p.sp, p.tr) as posed:
        skinned.set_skin(*d.steps[0][1:])
        posed.set_parts(*p.steps[0][1:])
        for step in (1, 2, 3):
            skinned.skin(d.steps[step][1])
            posed.pose(p.steps[step][1])
            a, b = skinned.export_bvh(), posed.export_bvh()
            for k in TREE_KEYS:
                _same("rigid step %d: exported %s against the posed twin's" % (step, k), a[k], b[k])
            _same("rigid step %d: read_triangles against the posed twin's" % step, skinned.read_triangles(), posed.read_triangles())


def test_keep_preserves_minus_zero_and_the_nan_payload_on_the_device(hpt, torch):
    d = sc.data("keep")
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        for step in range(3):
            _apply(torch, scene, "keep", step)
            got = scene.read_triangles()
            assert got.tobytes() == d.tr.tobytes(), step
        bits = po.verts_of(got).view(U32)
        assert bits[0, 1, 0] == 0x80000000 and bits[11, 2, 1] == 0x7FC12345
        _check_tree(hpt, scene, "keep", 2, hpt.export_bvh_host(d.L, d.sp, d.tr))          # ... and the builder's tree
        _apply(torch, scene, "keep", 3)                                                     # the sphere blends, the walls are kept
        bits = po.verts_of(scene.read_triangles()).view(U32)
        assert bits[0, 1, 0] == 0x80000000 and bits[11, 2, 1] == 0x7FC12345
        assert np.array_equal(bits[:sc.NWALL], po.verts_of(d.tr).view(U32)[:sc.NWALL])


# ---- the other integrators: the lazy host records -------------------------------------------------------------------------

def _bdpt(hpt, scene, d):
    cam = sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, sc.W, sc.H, tan_in_float=True)
    return scene.render_bdpt(cam, sc.W, sc.H, 4, 4, sc.SPP, 8, hpt.make_params(seed=3))


def _bdpt_oracle(oracle_mod, d, L, sp, tr):
    return oracle_mod.bdpt_render(L, sp, tr, d.order, d.eye, d.look, sio.CORNELL_UP, 50.0, sc.W, sc.H, 4, 4, sc.SPP, 8, seed=3)[0]


PPM = dict(eye_depth=4, light_depth=4, spp=1, spl=256, radius=0.07, seed=5)
# (name, step, photon mapping too): photon mapping where every vertex is finite, as in the pose suite
OTHERS = [("bend", 1, True), ("bend", 2, True), ("die-and-return", 1, False), ("die-and-return", 2, True)]


@pytest.mark.parametrize("name", ["bend", "die-and-return"])
def test_bdpt_ppm_and_guides_after_skins(hpt, torch, oracle_mod, tmp_path, name):
    """Groups set and the bidirectional scene built before the first step; then, after skins that nobody read back, BDPT
    and photon mapping with null bounds -- both built from the handle's host records, which a skin leaves behind the
    device's vertices -- and the guides."""
    d = sc.data(name)
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
            L, sp, tr = sc.records(name, step)
            got = scene.render_guides(sc.camera(name), sc.W, sc.H, sc.SPP, hpt.make_params(seed=5))
            want, _ = guides_oracle.render(glib, L, sp, tr, sc.camera(name), sc.W, sc.H, sc.SPP, seed=5)
            for k in GUIDE_KEYS:
                _same("%s: guide %s" % (where, k), got[k], want[k])
            _same(where + ": BDPT", _bdpt(hpt, scene, d), _bdpt_oracle(oracle_mod, d, L, sp, tr))
            if with_ppm:
                got = scene.render_ppm(sc.camera(name), sc.W, sc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"],
                                       hpt.make_params(seed=kw["seed"]))
                want = ppm_oracle.render(plib, L, sp, tr, sc.camera(name), sc.W, sc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"],
                                         kw["radius"], seed=kw["seed"])[0]
                _same(where + ": PPM with null bounds", got, want)


# ---- motion ------------------------------------------------------------------------------------------------------------

def test_the_per_frame_chain_of_motion_on_skins(hpt, tmp_path):
    """The base sphere bent further every frame: skin, render_guides(prev_position=True), keep_previous.  prev_position is
    motion_oracle's bytes, and on the pixels whose samples all end on the walls -- four zero weights -- it equals position
    bit for bit."""
    L, sp, tr0 = pc.base()
    bone, weight = sc.height_weights(tr0)
    mlib, glib = motion_oracle.build(tmp_path), guides_oracle.build(tmp_path)
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, sc.W, sc.H)
    walls_only, _ = guides_oracle.render(glib, L, sp, tr0[:sc.NWALL], cam, sc.W, sc.H, sc.SPP, seed=7)
    with hpt.Scene(L, sp, tr0) as scene:
        scene.set_skin(bone, weight, 2)
        assert not scene.has_motion()                              # set_skin changes no geometry
        prev = tr0
        for frame, deg in enumerate((0.0, 25.0, 50.0, 75.0)):
            xf = sc.twist(deg, rc.SPHERE_C) if frame else pc.identity(2)
            scene.skin(xf)
            tr = so.skin(tr0, bone, weight, xf)
            assert scene.has_motion()
            got = scene.render_guides(cam, sc.W, sc.H, sc.SPP, hpt.make_params(seed=7), prev_position=True)
            want, _ = motion_oracle.render(mlib, L, sp, tr, sp, prev, cam, sc.W, sc.H, sc.SPP, seed=7)
            for k in motion_oracle.KEYS:
                a, b = got[k], want[k]
                bad = (a.view(U32) != b.view(U32)) & ~(np.isnan(a) & np.isnan(b))
                assert not bad.any(), ("frame %d: guide %s" % (frame, k), int(bad.sum()))
            wall = (got["position"].view(U32) == walls_only["position"].view(U32)).all(axis=-1) & (got["coverage"] > 0)
            assert wall.mean() > 0.5
            assert np.array_equal(got["prev_position"].view(U32)[wall], got["position"].view(U32)[wall]), frame
            moved = (got["prev_position"].view(U32) != got["position"].view(U32)).any(axis=-1)
            if frame == 0:
                assert not moved.any()                             # every bone at identity: keep, the same bits
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
    for w in words:
        assert w in msg, msg


def test_refused_calls_leave_the_handle_as_it_was(hpt, torch, oracle_mod):
    name = "bend"
    d = sc.data(name)
    n = len(d.tr)
    _, bone, weight, nb = d.steps[0]
    good = d.steps[1][1]
    lib = hpt.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def edited(a, at, value):
        a = a.copy(); a[at] = value
        return a
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _refused(hpt, lambda: scene.skin(good), "before hpt_scene_set_skin")
        scene.set_parts(None, 1)
        _refused(hpt, lambda: scene.skin(good), "before hpt_scene_set_skin")
        scene.set_skin(bone, weight, nb)
        _refused(hpt, lambda: scene.pose(pc.identity(1)), "before hpt_scene_set_parts")           # one deformer per scene
        assert not scene.has_motion()
        scene.skin(good)
        want_img, want_tree, info = _pt(hpt, scene, name), scene.export_bvh(), scene.update_info()
        _refused(hpt, lambda: scene.set_skin(bone[:-1], weight[:-1], nb), "count")
        _refused(hpt, lambda: scene.set_skin(bone, weight[:-1], nb), "four bones and four weights")
        _refused(hpt, lambda: scene.set_skin(bone, weight, 0), "bones")
        _refused(hpt, lambda: scene.set_skin(bone, weight, 65537), "bones")
        _refused(hpt, lambda: scene.set_skin(edited(bone, (40, 1, 2), 2), weight, nb), "triangle 40 corner 1")
        _refused(hpt, lambda: scene.set_skin(edited(bone, (3, 0, 0), -1), weight, nb), "triangle 3 corner 0")       # weightless, still refused
        for bad in (-0.0, -1.0, float("nan"), float("inf")):
            _refused(hpt, lambda: scene.set_skin(bone, edited(weight, (50, 2, 3), bad), nb), "triangle 50 corner 2", "negative or not finite")
        assert lib.hpt_scene_set_skin(scene._h, None, vp(weight), n, nb) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_set_skin(scene._h, vp(bone), None, n, nb) == 1 and b"null" in lib.hpt_last_error()
        _refused(hpt, lambda: scene.skin(pc.identity(3)), "bones")
        _refused(hpt, lambda: scene.skin(pc.identity(1)), "bones")
        assert lib.hpt_scene_skin(scene._h, None, nb) == 1 and b"null" in lib.hpt_last_error()
        if hpt.device_count() >= 2:
            torch.cuda.set_device(1)
            try:
                _refused(hpt, lambda: scene.skin(good), "another device")
                _refused(hpt, lambda: scene.set_skin(bone, weight, nb), "another device")
            finally:
                torch.cuda.set_device(0)
        # ... the handle is as it was: the influences and the rest pose too (the next skin gives the expected scene)
        assert scene.update_info() == info
        _same("after the refusals: render_pt", _pt(hpt, scene, name), want_img)
        got_tree = scene.export_bvh()
        for k in TREE_KEYS:
            _same("after the refusals: exported " + k, got_tree[k], want_tree[k])
        scene.skin(d.steps[2][1])
        _check_tree(hpt, scene, name, 2)
        _same("after the refusals: the next skin", _pt(hpt, scene, name), sc.scan(oracle_mod, name, 2)[0])


def test_a_scene_of_no_triangles_takes_every_call_with_zero_counts(hpt, torch):
    d = sc.data("bend")
    empty = d.tr[:0]
    none_b, none_w = sc.no_weights(0)
    with hpt.Scene(d.L, d.sp, empty) as scene:
        scene.set_skin(none_b, none_w, 1)
        scene.skin(pc.identity(1))
        scene.set_skin(none_b, none_w, 65536)
        scene.skin(pc.identity(65536))
        assert len(scene.read_triangles()) == 0
        assert len(hpt.skin_host(empty, none_b, none_w, pc.identity(2))) == 0
        assert scene.update_info()["updates"] == 2
        dev, host = scene.export_bvh(), hpt.export_bvh_host(d.L, d.sp, empty)
        for k in TREE_KEYS:
            _same("no triangles: exported " + k, dev[k], host[k])


# ---- CLI ------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(CSRC, "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_twist_device_reproject_keeps_history(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    obj = str(tmp_path / "mesh.obj")
    sio.write_obj(obj, sio._tris_from(sio.tessellated_sphere((-0.15, 0.25, 0.0), 0.15, 12, 12), np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), np.float32), (264, 1))))
    base = ["--mode", "pt", "--input", scene_file, "--obj", obj, "--seed", 13, "--width", 64, "--height", 48, "--frame-spp", 2, "--guide-spp", 3,
            "--output", tmp_path / "out.png"]
    run = _cli(*base, "--frames", 3, "--twist-device", 5, "--reproject")
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    kept = [float(v) for v in re.findall(r"^\[Frame \d+\] rms \S+ kept (\S+) %$", run.stdout, flags=re.M)]
    assert len(kept) == 3 and kept[0] == 0.0 and all(v > 0.0 for v in kept[1:]), run.stdout
    for other in ("--spin", "--spin-device"):
        out = tmp_path / ("x%s.png" % other)
        run = _cli(*base[:-1], out, "--frames", 3, "--twist-device", 5, other, 5)
        assert run.returncode != 0 and "exclude each other" in run.stderr, other
        assert not os.path.exists(out)
    run = _cli("--mode", "pt", "--input", scene_file, "--output", tmp_path / "y.png", "--twist-device", 5, "--frames", 2)
    assert run.returncode != 0 and "--twist-device needs --frames and --obj" in run.stderr
    assert not os.path.exists(tmp_path / "y.png")
