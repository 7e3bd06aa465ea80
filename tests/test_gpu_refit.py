"""Scene updates on the MI355X: every case of refit_cases.py on ONE long-lived handle, updated step after step with
Scene.update_triangles / Scene.update_rounds.  After every step the device's tree is held to the bytes of the host
definition (path_tracing_amd.refit_bvh_host from the base scene: a refit is a function of the topology and the new
vertices alone) and the path tracer to the oracle's scan of the new records under every way it walks the tree: default,
trace budget 1 (every ray through the four-wide resume walk), budget 63 (no split), brute force and the counting
kernels, whose work counts must be the oracle's host walk of the exported tree.  The probes exercise the float twin of
the tree.  BDPT (groups set before the updates), photon mapping with the scene's own bounds and the guides are held to
their oracles after an update; tests/test_refit_cpu.py keeps every step's image distinct from the one before, so a
structure left stale cannot pass.  Every render is 48 x 48, 4 spp."""
import numpy as np
import pytest

import guides_oracle
import ppm_oracle
import refit_cases as rc
from path_tracing_amd import scene_io as sio
from test_bvh_walk import COUNT_KEYS

pytestmark = pytest.mark.gpu

TREE_KEYS = ("num_nodes", "num_tris", "bvh_depth", "num_rounds", "qorigin", "qscale", "qnodes", "tris")
GUIDE_KEYS = ("albedo", "normal", "position", "coverage")
SHAPE_STATS = ("bvh_nodes", "bvh_depth", "n_tris", "n_materials", "ms_bvh_build", "ms_upload")
N_PROBE = 4096


def _same(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        bits = "u%d" % got.dtype.itemsize
        diff = np.argwhere(got.view(bits) != want.view(bits))
        at = tuple(int(v) for v in diff[0])
        pytest.fail("%s differs in %d of %d values, first at %s: got %r, expected %r" % (what, len(diff), got.size, at, got[at].item(), want[at].item()))


def _params(hpt, flags=0, budget=0, seed=rc.SEED):
    p = hpt.make_params(seed=seed, flags=flags)
    p.reserved = budget << 1
    return p


def _pt(hpt, scene, name, flags=0, budget=0):
    return scene.render_pt(rc.camera(name), rc.W, rc.H, rc.DEPTH, rc.SPP, _params(hpt, flags, budget))


def _apply(scene, name, step):
    """The update that takes the handle from the records after step - 1 to those after `step`."""
    L, sp, tr = rc.records(name, step)
    if rc.is_rounds_step(name, step):
        scene.update_rounds(L, sp)
    if rc.is_triangle_step(name, step):
        scene.update_triangles(tr)


def _probe_rays(tr, seed):
    """N_PROBE seeded segments inside the live triangles' bounds (the unit cube when there are none)."""
    v = rc.verts(tr)[~rc.dead(tr)].reshape(-1, 3)
    lo, hi = (v.min(axis=0), v.max(axis=0)) if len(v) else (np.zeros(3), np.ones(3))
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (N_PROBE, 3)).astype(np.float32)
    p2 = rng.uniform(lo, hi, (N_PROBE, 3)).astype(np.float32)
    d = p2.astype(np.float64) - o
    d = (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    return o, d, p2


def _check_tree(hpt, scene, name, step):
    dev, host = scene.export_bvh(), rc.tree(hpt, name, step)
    for k in TREE_KEYS:
        _same("%s step %d: exported %s" % (name, step, k), dev[k], host[k])
    return dev


def _check_step(hpt, oracle_mod, scene, name, step):
    where = "%s step %d" % (name, step)
    L, sp, tr = rc.records(name, step)
    dev = _check_tree(hpt, scene, name, step)
    scan, _ = rc.scan(oracle_mod, name, step)
    for what, flags, budget in (("default", 0, 0), ("budget 1", 0, 1), ("budget 63", 0, 63), ("brute force", hpt.FLAG_BRUTE_FORCE, 0)):
        _same("%s: render_pt, %s" % (where, what), _pt(hpt, scene, name, flags, budget), scan)
    _same("%s: render_pt, counting" % where, _pt(hpt, scene, name, hpt.FLAG_COUNT_WORK), scan)
    st = scene.stats()
    walk, so = oracle_mod.pt_render(L, sp, tr, rc.camera(name), rc.W, rc.H, rc.DEPTH, rc.SPP, seed=rc.SEED, bvh=dev)
    assert np.array_equal(walk, scan), where
    assert {k: int(st[k]) for k in COUNT_KEYS} == {k: int(so[k]) for k in COUNT_KEYS}, where
    # the probes walk the float nodes
    o, d, p2 = _probe_rays(tr, 100 + step)
    t, prim = scene.trace_closest(o, d)
    tb, primb = scene.trace_closest(o, d, brute_force=True)
    to, primo = oracle_mod.closest_hits(L, sp, tr, o, d)
    _same(where + ": trace_closest prim against brute force", prim, primb)
    _same(where + ": trace_closest t against brute force", t, tb)
    _same(where + ": trace_closest prim against the oracle", prim, primo)
    _same(where + ": trace_closest t against the oracle", t, to)
    vis = scene.trace_visibility(o, p2)
    _same(where + ": trace_visibility against brute force", vis, scene.trace_visibility(o, p2, brute_force=True))
    _same(where + ": trace_visibility against the oracle", vis, oracle_mod.visibility(sp, tr, o, p2))


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_on_one_handle(hpt, oracle_mod, name):
    """Tree bytes, the five PT renders, the work counts and the probes after every step of the case."""
    d = rc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _same(name + ": base render", _pt(hpt, scene, name), rc.scan(oracle_mod, name, -1)[0])       # workspaces exist before the first update
        shape = {k: scene.stats()[k] for k in SHAPE_STATS}
        for step in range(len(d.steps)):
            _apply(scene, name, step)
            _check_step(hpt, oracle_mod, scene, name, step)
            info = scene.update_info()
            if rc.is_triangle_step(name, step):
                n_dead = int(rc.dead(rc.records(name, step)[2]).sum())
                assert (info["dead_tris"], info["live_tris"]) == (n_dead, len(d.tr) - n_dead), (name, step)
            assert info["updates"] == sum(rc.is_triangle_step(name, s) for s in range(step + 1))
            assert {k: scene.stats()[k] for k in SHAPE_STATS} == shape, (name, step)


def test_update_info_counts_the_dead_of_die_and_return(hpt):
    name = "die-and-return"
    d = rc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        assert scene.update_info() == dict(updates=0, live_tris=0, dead_tris=0, ms_pack=0.0, ms_upload=0.0, ms_refit=0.0)
        for step in range(len(d.steps)):
            scene.update_triangles(rc.records(name, step)[2])
            info = scene.update_info()
            assert (info["updates"], info["dead_tris"], info["live_tris"]) == (step + 1, rc.N_DEAD[(name, step)], 1872 - rc.N_DEAD[(name, step)])
            assert info["ms_refit"] > 0 and info["ms_pack"] >= 0 and info["ms_upload"] > 0


# ---- the other integrators after an update -------------------------------------------------------------------------------

def _bdpt(hpt, scene, d, name, seed=3):
    cam = sio.make_camera(d.eye, d.look, sio.CORNELL_UP, 50.0, rc.W, rc.H, tan_in_float=True)
    return scene.render_bdpt(cam, rc.W, rc.H, 4, 4, rc.SPP, 8, hpt.make_params(seed=seed))


def _bdpt_oracle(oracle_mod, d, L, sp, tr, seed=3):
    return oracle_mod.bdpt_render(L, sp, tr, d.order, d.eye, d.look, sio.CORNELL_UP, 50.0, rc.W, rc.H, 4, 4, rc.SPP, 8, seed=seed)[0]


def test_bdpt_after_updates_keeps_the_groups(hpt, oracle_mod):
    """turn: the groups are set and the bidirectional scene is built (a render) before the first update."""
    name = "turn"
    d = rc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        scene.set_groups(*d.order)
        _same("turn: BDPT of the base scene", _bdpt(hpt, scene, d, name), _bdpt_oracle(oracle_mod, d, d.L, d.sp, d.tr))
        for step in (0, 1):
            L, sp, tr = rc.records(name, step)
            scene.update_triangles(tr)
            want = _bdpt_oracle(oracle_mod, d, L, sp, tr)
            assert rc.changed_share(want, _bdpt_oracle(oracle_mod, d, *rc.records(name, step - 1))) >= 0.05
            _same("turn step %d: BDPT" % step, _bdpt(hpt, scene, d, name), want)


def test_ppm_with_null_bounds_uses_the_new_bounds(hpt, tmp_path):
    name, step = rc.PPM_STEP
    d, (L, sp, tr) = rc.data(name), rc.records(name, step)
    lib = ppm_oracle.build(tmp_path)
    kw = dict(rc.PPM)

    def device(scene):
        return scene.render_ppm(rc.camera(name), rc.W, rc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"],
                                hpt.make_params(seed=kw["seed"]))

    def oracle(records):
        return ppm_oracle.render(lib, *records, rc.camera(name), rc.W, rc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"],
                                 seed=kw["seed"])[0]

    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        _same("parallel: PPM of the base scene", device(scene), oracle((d.L, d.sp, d.tr)))            # the base scene's bounds are in use
        scene.update_triangles(tr)
        _same("parallel step 0: PPM", device(scene), oracle((L, sp, tr)))


def test_guides_after_an_update(hpt, tmp_path):
    name = "turn"
    d = rc.data(name)
    lib = guides_oracle.build(tmp_path)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        for step in (-1, 0):
            L, sp, tr = rc.records(name, step)
            if step >= 0:
                scene.update_triangles(tr)
            got = scene.render_guides(rc.camera(name), rc.W, rc.H, rc.SPP, hpt.make_params(seed=5))
            want, _ = guides_oracle.render(lib, L, sp, tr, rc.camera(name), rc.W, rc.H, rc.SPP, seed=5)
            for k in GUIDE_KEYS:
                _same("turn step %d: guide %s" % (step, k), got[k], want[k])


def test_update_rounds_for_pt_and_bdpt(hpt, oracle_mod):
    """rounds: the light moved and dimmed, one sphere moved and one grown; then the triangles as well."""
    name = "rounds"
    d = rc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        scene.set_groups(*d.order)
        _same("rounds: BDPT of the base scene", _bdpt(hpt, scene, d, name), _bdpt_oracle(oracle_mod, d, d.L, d.sp, d.tr))
        for step in range(len(d.steps)):
            L, sp, tr = rc.records(name, step)
            _apply(scene, name, step)
            _same("rounds step %d: PT" % step, _pt(hpt, scene, name), rc.scan(oracle_mod, name, step)[0])
            _same("rounds step %d: BDPT" % step, _bdpt(hpt, scene, d, name), _bdpt_oracle(oracle_mod, d, L, sp, tr))


# ---- the handle ------------------------------------------------------------------------------------------------------

def test_an_update_between_two_renders_leaves_the_scene_statistics(hpt, oracle_mod):
    name = "there-and-back"
    d = rc.data(name)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        first = _pt(hpt, scene, name, hpt.FLAG_COUNT_WORK)
        before = scene.stats()
        scene.update_triangles(rc.records(name, 0)[2])
        _same("there-and-back step 0", _pt(hpt, scene, name, hpt.FLAG_COUNT_WORK), rc.scan(oracle_mod, name, 0)[0])
        after = scene.stats()
        for k in ("bvh_nodes", "bvh_depth", "n_tris", "n_materials", "ms_bvh_build"):
            assert after[k] == before[k], k
        assert after["closest_rays"] != before["closest_rays"]                 # ... while the render's own are the new render's
        scene.update_triangles(rc.records(name, 1)[2])
        _same("there-and-back step 1 against the first render", _pt(hpt, scene, name, hpt.FLAG_COUNT_WORK), first)
        assert {k: scene.stats()[k] for k in COUNT_KEYS} == {k: before[k] for k in COUNT_KEYS}     # the builder's tree again


def _refused(hpt, call, *words):
    with pytest.raises(hpt.HptError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith("hpt error 1:"), msg
    for w in words:
        assert w in msg, msg


def test_refused_updates_leave_the_handle_as_it_was(hpt, oracle_mod):
    """Every refusal through update_check and through the updates themselves; afterwards the handle renders the previous
    scene's bytes and exports the previous tree.  (The refusal for a current device other than the scene's is made where
    the machine shows two devices.)"""
    name = "rounds"
    d = rc.data(name)
    L1, sp1, tr1 = rc.records(name, 1)
    with hpt.Scene(d.L, d.sp, d.tr) as scene:
        scene.update_triangles(tr1)
        want_img, want_tree = _pt(hpt, scene, name), scene.export_bvh()
        info = scene.update_info()
        bad_mat = tr1.copy()
        col = bad_mat["mtl"]["base_color"].copy(); col[7] = (0.1, 0.2, 0.3); bad_mat["mtl"]["base_color"] = col
        bad_id = tr1.copy(); bad_id["id"][5] = 99999
        for call in (scene.update_check, scene.update_triangles):
            _refused(hpt, lambda: call(tr1[:-1]), "count")
            _refused(hpt, lambda: call(np.concatenate([tr1, tr1[:1]])), "count")
            _refused(hpt, lambda: call(bad_mat), "triangle 7")
            _refused(hpt, lambda: call(bad_id), "triangle 5")
        lib = hpt.load_library()
        assert lib.hpt_scene_update_triangles(scene._h, None, len(tr1)) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_update_check(scene._h, None, len(tr1)) == 1 and b"null" in lib.hpt_last_error()
        assert lib.hpt_scene_update_triangles(None, None, 0) == 1 and b"null scene" in lib.hpt_last_error()
        assert lib.hpt_scene_update_rounds(None, None, 0, None, 0) == 1 and b"null scene" in lib.hpt_last_error()
        assert lib.hpt_scene_update_rounds(scene._h, None, len(d.L), None, len(d.sp)) == 1 and b"null" in lib.hpt_last_error()
        _refused(hpt, lambda: scene.update_rounds(d.L[:0], d.sp), "counts")
        _refused(hpt, lambda: scene.update_rounds(d.L, d.sp[:1]), "counts")
        bad_sp = d.sp.copy(); bad_sp[1]["mtl"]["roughness"] = 0.25
        _refused(hpt, lambda: scene.update_rounds(d.L, bad_sp), "sphere 1")
        if hpt.device_count() >= 2:
            import torch
            torch.cuda.set_device(1)
            try:
                _refused(hpt, lambda: scene.update_check(tr1), "another device")
                _refused(hpt, lambda: scene.update_triangles(tr1), "another device")
                _refused(hpt, lambda: scene.update_rounds(d.L, d.sp), "another device")
            finally:
                torch.cuda.set_device(0)
        scene.update_check(tr1)                                               # ... and what is right is accepted
        assert scene.update_info() == info
        _same("after the refusals: render_pt", _pt(hpt, scene, name), want_img)
        got_tree = scene.export_bvh()
        for k in TREE_KEYS:
            _same("after the refusals: exported " + k, got_tree[k], want_tree[k])
        _same("after the refusals: the scene is step 1 without the rounds update", want_img,
              oracle_mod.pt_render(d.L, d.sp, tr1, rc.camera(name), rc.W, rc.H, rc.DEPTH, rc.SPP, seed=rc.SEED)[0])


def test_a_scene_of_no_triangles_takes_an_update_of_none(hpt, oracle_mod):
    d = rc.data("rounds")
    L1, sp1, _ = rc.records("rounds", 0)
    with hpt.Scene(d.L, d.sp, d.tr[:0]) as scene:
        scene.update_triangles(d.tr[:0])
        scene.update_rounds(L1, sp1)
        dev, host = scene.export_bvh(), hpt.export_bvh_host(L1, sp1, d.tr[:0])
        for k in TREE_KEYS:
            _same("no triangles: exported " + k, dev[k], host[k])
        _same("no triangles: render_pt", _pt(hpt, scene, "rounds"),
              oracle_mod.pt_render(L1, sp1, d.tr[:0], rc.camera("rounds"), rc.W, rc.H, rc.DEPTH, rc.SPP, seed=rc.SEED)[0])
