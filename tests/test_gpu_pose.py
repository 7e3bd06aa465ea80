"""Poses on the MI355X (include/hpt.h, "poses"): every case of pose_cases.py on ONE long-lived handle, step after step
through Scene.set_parts, Scene.pose, Scene.update_triangles and Scene.update_vertices_device.  After every step the
exported tree is held to the bytes of hpt_bvh_refit_host of the records pose_oracle expects, Scene.read_triangles to those
records, and the path tracer to the oracle's scan of them under every way it walks the tree.  The lazy host-record paths
(the bidirectional scene, photon mapping's own bounds) and the guides are held to their oracles after poses; the per-frame
chain of "motion" runs on poses; the refusals leave the handle as it was; pt_cli --spin-device runs.
tests/test_pose_cpu.py keeps every step's image distinct from the one before and `turn` sensitive to contraction."""
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
from path_tracing_amd import scene_io as sio

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "path_tracing_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")
TREE_KEYS = ("num_nodes", "num_tris", "bvh_depth", "num_rounds", "qorigin", "qscale", "qnodes", "tris")
GUIDE_KEYS = ("albedo", "normal", "position", "coverage")


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


def _params(hpt, flags=0, budget=0, seed=pc.SEED):
    p = hpt.make_params(seed=seed, flags=flags)
    p.reserved = budget << 1
    return p


def _pt(hpt, scene, name, flags=0, budget=0):
    return scene.render_pt(pc.camera(name), pc.W, pc.H, pc.DEPTH, pc.SPP, _params(hpt, flags, budget))


def _device_verts(torch, tr, flat):
    v = torch.from_numpy(po.verts_of(tr)).cuda()
    return v.reshape(-1) if flat else v


def _apply(torch, scene, name, step):
    s = pc.data(name).steps[step]
    if s[0] == "parts":
        scene.set_parts(s[1], s[2])
    elif s[0] == "pose":
        scene.pose(s[1])
    elif s[0] == "tris":
        scene.update_triangles(s[1])
    else:
        scene.update_vertices_device(_device_verts(torch, s[1], flat=step % 2 == 1))


def _check_tree(hpt, scene, name, step, want=None):
    dev, host = scene.export_bvh(), want or pc.tree(hpt, name, step)
    for k in TREE_KEYS:
        _same("%s step %d: exported %s" % (name, step, k), dev[k], host[k])


# ---- every case on one handle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.NAMES)
def test_case_on_one_handle(hpt, torch, oracle_mod, name):
    """Tree bytes, read_triangles, the four PT renders and the update counts after every step of the case."""
    d = pc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _same(name + ": base render", _pt(hpt, scene, name), pc.scan(oracle_mod, name, -1)[0])       # workspaces exist before the first update
        updates = 0
        for step in range(len(d.steps)):
            where = "%s step %d" % (name, step)
            _apply(torch, scene, name, step)
            tr = pc.records(name, step)[2]
            _check_tree(hpt, scene, name, step)
            info = scene.update_info()
            if pc.is_geometry_step(name, step):
                updates += 1
                n_dead = int(rc.dead(tr).sum())
                assert (info["dead_tris"], info["live_tris"]) == (n_dead, len(tr) - n_dead), where
                if (name, step) in pc.N_DEAD:
                    assert n_dead == pc.N_DEAD[(name, step)]
                if d.steps[step][0] != "tris":
                    assert info["ms_pack"] == 0.0 and info["ms_upload"] > 0 and info["ms_refit"] > 0, where
            assert info["updates"] == updates, where
            scan = pc.scan(oracle_mod, name, step)[0]
            for what, flags, budget in (("default", 0, 0), ("budget 1", 0, 1), ("budget 63", 0, 63), ("brute force", hpt.FLAG_BRUTE_FORCE, 0)):
                _same("%s: render_pt, %s" % (where, what), _pt(hpt, scene, name, flags, budget), scan)
            _same(where + ": read_triangles", scene.read_triangles(), tr)
        if name.startswith("dv-"):                                # ... and the trees are update_triangles' own
            src = name[3:]
            _check_tree(hpt, scene, name, len(d.steps) - 1, rc.tree(hpt, src, len(d.steps) - 1))


def test_identity_keeps_the_builders_tree_and_minus_zero(hpt, torch):
    d = pc.data("identity")
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        for step in range(len(d.steps)):
            _apply(torch, scene, "identity", step)
        _check_tree(hpt, scene, "identity", 1, hpt.export_bvh_host(d.L, d.sp, d.tr))
        got = scene.read_triangles()
        assert got.tobytes() == d.tr.tobytes() and np.signbit(got["v1"][0, 0])


# ---- the other integrators: the lazy host records -------------------------------------------------------------------------

def _bdpt(hpt, scene, d):
    cam = sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, pc.W, pc.H, tan_in_float=True)
    return scene.render_bdpt(cam, pc.W, pc.H, 4, 4, pc.SPP, 8, hpt.make_params(seed=3))


def _bdpt_oracle(oracle_mod, d, L, sp, tr):
    return oracle_mod.bdpt_render(L, sp, tr, d.order, d.eye, d.look, sio.CORNELL_UP, 50.0, pc.W, pc.H, 4, 4, pc.SPP, 8, seed=3)[0]


PPM = dict(eye_depth=4, light_depth=4, spp=1, spl=256, radius=0.07, seed=5)
# (name, step, photon mapping too): photon mapping where every vertex is finite -- the bounds of records with NaN in them
# depend on how a maximum treats NaN, which the definition of the bounds leaves to the reference's helper
OTHERS = [("turn", 1, True), ("turn", 2, True), ("die-and-return", 1, False), ("die-and-return", 2, True)]


@pytest.mark.parametrize("name", ["turn", "die-and-return"])
def test_bdpt_ppm_and_guides_after_poses(hpt, torch, oracle_mod, tmp_path, name):
    """Groups set and the bidirectional scene built before the first step; then, after poses that nobody read back, BDPT
    and photon mapping with null bounds -- both built from the handle's host records, which a pose leaves behind the
    device's vertices -- and the guides."""
    d = pc.data(name)
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
            L, sp, tr = pc.records(name, step)
            got = scene.render_guides(pc.camera(name), pc.W, pc.H, pc.SPP, hpt.make_params(seed=5))
            want, _ = guides_oracle.render(glib, L, sp, tr, pc.camera(name), pc.W, pc.H, pc.SPP, seed=5)
            for k in GUIDE_KEYS:
                _same("%s: guide %s" % (where, k), got[k], want[k])
            _same(where + ": BDPT", _bdpt(hpt, scene, d), _bdpt_oracle(oracle_mod, d, L, sp, tr))
            if with_ppm:
                got = scene.render_ppm(pc.camera(name), pc.W, pc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"],
                                       hpt.make_params(seed=kw["seed"]))
                want = ppm_oracle.render(plib, L, sp, tr, pc.camera(name), pc.W, pc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"],
                                         kw["radius"], seed=kw["seed"])[0]
                _same(where + ": PPM with null bounds", got, want)


def test_ppm_with_null_bounds_follows_a_pose(hpt, tmp_path):
    """refit_cases' parallel-light scene, whose image depends on the bounds: posed as one part (a null map)."""
    name, step = rc.PPM_STEP
    d = rc.data(name)
    lib = ppm_oracle.build(tmp_path)
    kw = dict(rc.PPM)
    rec = pc.table(pc.affine(pc.rot_z(60.0) * 0.7, shift=(0.15, 0.1, -0.2)))
    want_tr = po.pose(d.tr, None, rec)

    def device(scene):
        return scene.render_ppm(rc.camera(name), rc.W, rc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"],
                                hpt.make_params(seed=kw["seed"]))

    def oracle(tr):
        return ppm_oracle.render(lib, d.L, d.sp, tr, rc.camera(name), rc.W, rc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"],
                                 seed=kw["seed"])[0]

    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _same("parallel: PPM of the base scene", device(scene), oracle(d.tr))
        scene.set_parts(None, 1)
        scene.pose(rec)
        _same("parallel posed: PPM", device(scene), oracle(want_tr))


# ---- motion ------------------------------------------------------------------------------------------------------------

def test_the_per_frame_chain_of_motion_on_poses(hpt, tmp_path):
    """turn: pose, render_guides_motion, keep_previous per frame.  prev_position is motion_oracle's bytes, and on the pixels
    whose samples all end on the walls -- part 0, left at identity -- it equals position bit for bit."""
    name = "turn"
    d = pc.data(name)
    mlib, glib = motion_oracle.build(tmp_path), guides_oracle.build(tmp_path)
    cam = pc.camera(name)
    walls_only, _ = guides_oracle.render(glib, d.L, d.sp, d.tr[:pc.NWALL], cam, pc.W, pc.H, pc.SPP, seed=7)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        prev = d.tr
        for step in range(len(d.steps)):
            _apply(None, scene, name, step)
            tr = pc.records(name, step)[2]
            assert scene.has_motion() == (step > 0)
            got = scene.render_guides(cam, pc.W, pc.H, pc.SPP, hpt.make_params(seed=7), prev_position=True)
            want, _ = motion_oracle.render(mlib, d.L, d.sp, tr, d.sp, prev, cam, pc.W, pc.H, pc.SPP, seed=7)
            for k in motion_oracle.KEYS:
                a, b = got[k], want[k]
                bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
                assert not bad.any(), ("step %d: guide %s" % (step, k), int(bad.sum()))
            wall = (got["position"].view(np.uint32) == walls_only["position"].view(np.uint32)).all(axis=-1) & (got["coverage"] > 0)
            assert wall.mean() > 0.5
            assert np.array_equal(got["prev_position"].view(np.uint32)[wall], got["position"].view(np.uint32)[wall]), step
            if step > 0:
                moved = (got["prev_position"].view(np.uint32) != got["position"].view(np.uint32)).any(axis=-1)
                assert moved.mean() > 0.02, step
            scene.keep_previous()
            assert not scene.has_motion()
            prev = tr


# ---- device vertices ------------------------------------------------------------------------------------------------------

def test_update_vertices_device_from_a_side_stream_and_from_a_pointer(hpt, torch, oracle_mod):
    """Vertices that a torch kernel on a side stream produced (the call waits for them), and the same through an integer
    pointer with a count; the handle then holds torch's own float32 results."""
    name = "turn"
    d = pc.data(name)
    rest = torch.from_numpy(po.verts_of(d.tr)).cuda()
    rec = torch.from_numpy(np.ascontiguousarray(pc.affine(pc.tilted(30.0), rc.SPHERE_C))).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        with torch.cuda.stream(side):
            v = rest.clone()
            for _ in range(20):                                    # enough work that the stream is still busy at the call
                turned = v[pc.NWALL:] @ rec[:, :3].T + rec[:, 3]
            v[pc.NWALL:] = turned
            v = v.contiguous()
        scene.update_vertices_device(v)
        want = po.with_verts(d.tr, v.cpu().numpy())
        _same("side stream: read_triangles", scene.read_triangles(), want)
        tree = hpt.refit_bvh_host(d.L, d.sp, d.tr, want)
        _check_tree(hpt, scene, name, 0, tree)
        img = _pt(hpt, scene, name)
        _same("side stream: render_pt", img, oracle_mod.pt_render(d.L, d.sp, want, pc.camera(name), pc.W, pc.H, pc.DEPTH, pc.SPP, seed=pc.SEED)[0])
        assert rc.changed_share(img, pc.scan(oracle_mod, name, -1)[0]) >= 0.05
        # back to the base through a pointer
        torch.cuda.synchronize()
        scene.update_vertices_device(rest.data_ptr(), len(d.tr))
        _same("pointer: read_triangles", scene.read_triangles(), d.tr)
        _check_tree(hpt, scene, name, -1)
        assert scene.update_info()["updates"] == 2


# ---- refusals -------------------------------------------------------------------------------------------------------------

def _refused(hpt, call, *words):
    with pytest.raises(hpt.HptError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith("hpt error 1:"), msg
    for w in words:
        assert w in msg, msg


def test_refused_calls_leave_the_handle_as_it_was(hpt, torch, oracle_mod):
    name = "turn"
    d = pc.data(name)
    n = len(d.tr)
    part = pc.two_parts(n)
    good = d.steps[1][1]
    lib = hpt.load_library()
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _refused(hpt, lambda: scene.pose(good), "before hpt_scene_set_parts")
        scene.set_parts(part, 2)
        scene.pose(good)
        want_img, want_tree, info = _pt(hpt, scene, name), scene.export_bvh(), scene.update_info()
        v = _device_verts(torch, d.tr, flat=False)
        _refused(hpt, lambda: scene.update_vertices_device(v[:-1].contiguous()), "count")
        _refused(hpt, lambda: scene.update_vertices_device(v.data_ptr(), n + 1), "count")
        _refused(hpt, lambda: scene.update_vertices_device(v.double()), "float32")
        _refused(hpt, lambda: scene.update_vertices_device(v.cpu()), "CUDA")
        _refused(hpt, lambda: scene.update_vertices_device(v.reshape(-1, 9)), "shape")
        _refused(hpt, lambda: scene.update_vertices_device(v[:, :, :2]), "contiguous")
        assert lib.hpt_scene_update_vertices_device(scene._h, None, n) == 1 and b"null" in lib.hpt_last_error()
        _refused(hpt, lambda: scene.set_parts(part[:-1], 2), "count")
        _refused(hpt, lambda: scene.set_parts(part, 0), "parts")
        _refused(hpt, lambda: scene.set_parts(part, (1 << 20) + 1), "parts")
        _refused(hpt, lambda: scene.set_parts(None, 2), "null part map")
        bad = part.copy(); bad[40] = 2; bad[50] = -1
        _refused(hpt, lambda: scene.set_parts(bad, 2), "triangle 40")
        _refused(hpt, lambda: scene.pose(pc.identity(3)), "parts")
        _refused(hpt, lambda: scene.pose(pc.identity(1)), "parts")
        assert lib.hpt_scene_pose(scene._h, None, 2) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_read_triangles(scene._h, None, n) == 1 and b"null" in lib.hpt_last_error()
        out = np.zeros(n - 1, d.tr.dtype)
        assert lib.hpt_scene_read_triangles(scene._h, out.ctypes.data_as(C.c_void_p), n - 1) == 1 and b"count" in lib.hpt_last_error()
        if hpt.device_count() >= 2:
            torch.cuda.set_device(1)
            try:
                _refused(hpt, lambda: scene.pose(good), "another device")
                _refused(hpt, lambda: scene.set_parts(part, 2), "another device")
                _refused(hpt, lambda: scene.read_triangles(), "another device")
                _refused(hpt, lambda: scene.update_vertices_device(v.data_ptr(), n), "another device")
            finally:
                torch.cuda.set_device(0)
        # ... the handle is as it was: the part map and the rest pose too (the same pose gives the same scene)
        assert scene.update_info() == info
        _same("after the refusals: render_pt", _pt(hpt, scene, name), want_img)
        got_tree = scene.export_bvh()
        for k in TREE_KEYS:
            _same("after the refusals: exported " + k, got_tree[k], want_tree[k])
        scene.pose(d.steps[2][1])
        _check_tree(hpt, scene, name, 2)
        _same("after the refusals: the next pose", _pt(hpt, scene, name), pc.scan(oracle_mod, name, 2)[0])


def test_a_scene_of_no_triangles_takes_every_call_with_zero_counts(hpt, torch):
    d = pc.data("turn")
    empty = d.tr[:0]
    with hpt.Scene(d.L, d.sp, empty) as scene:
        scene.set_parts(None, 1)
        scene.pose(pc.identity(1))
        scene.set_parts(np.zeros(0, np.int32), 3)
        scene.pose(pc.identity(3))
        scene.update_vertices_device(torch.zeros((0, 3, 3), dtype=torch.float32, device="cuda"))
        scene.update_vertices_device(0, 0)
        assert len(scene.read_triangles()) == 0
        assert scene.update_info()["updates"] == 4
        dev, host = scene.export_bvh(), hpt.export_bvh_host(d.L, d.sp, empty)
        for k in TREE_KEYS:
            _same("no triangles: exported " + k, dev[k], host[k])


# ---- CLI ------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(CSRC, "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_spin_device_reproject_keeps_history(tmp_path):
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    obj = str(tmp_path / "mesh.obj")
    sio.write_obj(obj, sio._tris_from(sio.tessellated_sphere((-0.15, 0.25, 0.0), 0.15, 12, 12), np.tile(np.array((0.7, 0.7, 0.7, 1.0, 0.0, 0.0), np.float32), (264, 1))))
    base = ["--mode", "pt", "--input", scene_file, "--obj", obj, "--seed", 13, "--width", 64, "--height", 48, "--frame-spp", 2, "--guide-spp", 3,
            "--output", tmp_path / "out.png"]
    run = _cli(*base, "--frames", 3, "--spin-device", 5, "--reproject")
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    kept = [float(v) for v in re.findall(r"^\[Frame \d+\] rms \S+ kept (\S+) %$", run.stdout, flags=re.M)]
    assert len(kept) == 3 and kept[0] == 0.0 and all(v > 0.0 for v in kept[1:]), run.stdout
    run = _cli(*base, "--frames", 3, "--spin-device", 5, "--spin", 5)
    assert run.returncode != 0 and "exclude each other" in run.stderr
    run = _cli("--mode", "pt", "--input", scene_file, "--output", tmp_path / "x.png", "--spin-device", 5, "--frames", 2)
    assert run.returncode != 0 and "--spin-device needs --frames and --obj" in run.stderr
    assert not os.path.exists(tmp_path / "x.png")
