"""Scene updates on the host alone (refit_cases.py): the definition of a refit, path_tracing_amd.refit_bvh_host, held to
the builder -- refitting a tree to the vertices it was built from reproduces the builder's bytes -- and, after every
step of every case, to what any tree must be: well formed with the base tree's topology, every leaf's live triangles
inside its dequantised box and every child box inside its parent's, and rendering the scan's bytes when the oracle walks
it.  The table itself is held to its conditions (every step changes the image, so a stale device structure cannot pass
the GPU half, tests/test_gpu_refit.py), the refusals are made without a device, and the refit runs -- as a chain, the way
a live handle is updated -- in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bc
import ppm_oracle
import refit_cases as rc
from test_bvh_walk import _check_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
TREE_KEYS = ("num_nodes", "num_tris", "bvh_depth", "num_rounds", "qorigin", "qscale", "qnodes", "tris")
RAYS = ("closest_rays", "shadow_rays")
STEPS = rc.all_steps()
STEP_IDS = ["%s-%d" % s for s in STEPS]


def same_tree(a, b):
    """Byte equality of two exported trees (the grid as bits: a NaN or a signed zero counts)."""
    for k in TREE_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


# ---- the host refit against the builder ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_identity_refit_reproduces_the_builder_on_the_build_cases(hpt, name):
    """NaN, infinite and overflowing records, finite outliers and the non-finite grid included."""
    L, sp, tr = bc.CASE_BY_NAME[name].make()[:3]
    same_tree(hpt.refit_bvh_host(L, sp, tr, tr), bc.tree(hpt, name))


@pytest.mark.parametrize("name", rc.NAMES)
def test_identity_refit_reproduces_the_builder_on_the_base_scenes(hpt, name):
    d = rc.data(name)
    same_tree(hpt.refit_bvh_host(d.L, d.sp, d.tr, d.tr), rc.tree(hpt, name, -1))


def test_steps_that_return_to_the_base_scene_end_at_the_builders_bytes(hpt):
    """identity; there-and-back's last step; die-and-return's last step (after every triangle was dead).  The chain
    A -> B -> A itself runs in the sanitizer program below, which is held to these trees."""
    for name, step in (("identity", 0), ("there-and-back", 1), ("die-and-return", 3)):
        assert rc.records(name, step)[2].tobytes() == rc.data(name).tr.tobytes()
        same_tree(rc.tree(hpt, name, step), rc.tree(hpt, name, -1))


# ---- every step of every case ----------------------------------------------------------------------------------------

def _dequantised(bvh):
    """Per node and side the child's box in scene coordinates (float64): lo[n, side, axis], hi[n, side, axis]."""
    w = bvh["qnodes"][:, :6].astype(np.int64)
    qlo = np.stack([w[:, 0::2] & 0xFFFF, w[:, 0::2] >> 16], axis=1)          # [n, side, axis]
    qhi = np.stack([w[:, 1::2] & 0xFFFF, w[:, 1::2] >> 16], axis=1)
    o, s = bvh["qorigin"].astype(np.float64), bvh["qscale"].astype(np.float64)
    return qlo, qhi, o + qlo * s, o + qhi * s


@pytest.mark.parametrize("name,step", STEPS, ids=STEP_IDS)
def test_refitted_tree_is_well_formed_and_holds_its_triangles(hpt, name, step):
    base, bvh = rc.tree(hpt, name, -1), rc.tree(hpt, name, step)
    tr = rc.records(name, step)[2]
    _check_tree(bvh, len(tr))
    # the topology is the build's
    for k in ("num_nodes", "num_tris", "bvh_depth", "num_rounds"):
        assert bvh[k] == base[k], k
    assert np.array_equal(bvh["qnodes"][:, 6:8], base["qnodes"][:, 6:8])
    assert np.array_equal(bvh["tris"][:, [3, 7, 11]], base["tris"][:, [3, 7, 11]])          # ordinal, material, flags
    assert np.isfinite(bvh["qorigin"]).all() and np.isfinite(bvh["qscale"]).all() and (bvh["qscale"] > 0).all()
    # the records are the new vertices', bit for bit
    ords = bvh["tris"][:, 3].astype(np.int64) - bvh["num_rounds"]
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.concatenate([tr["v0"], tr["v1"] - tr["v0"], tr["v2"] - tr["v0"]], axis=1).astype(np.float32)[ords]
    got = bvh["tris"][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    live = ~rc.dead(tr)[ords]
    assert np.array_equal(got[live], want.view(np.uint32)[live])
    assert np.array_equal(np.isfinite(got.view(np.float32)), np.isfinite(want))
    # boxes: every leaf's live triangles inside its dequantised box, every inner child's two boxes inside its own
    qlo, qhi, lo, hi = _dequantised(bvh)
    v = rc.verts(tr)[ords]                                                    # [slot, vertex, axis]
    codes = bvh["qnodes"][:, 6:8].astype(np.int64)
    checked = 0
    for n in range(bvh["num_nodes"]):
        for side in (0, 1):
            c = int(codes[n, side])
            if c == 0xFFFFFFFF:
                assert (qlo[n, side] == 65535).all() and (qhi[n, side] == 0).all()
            elif c & 0x80000000:
                first, cnt = (c & 0x7FFFFFFF) >> 3, (c & 7) + 1
                for s in range(first, first + cnt):
                    if live[s]:
                        assert (v[s] >= lo[n, side]).all() and (v[s] <= hi[n, side]).all(), (n, side, s)
                        checked += 1
            else:
                kids = [k for k in (0, 1) if codes[c, k] != 0xFFFFFFFF]
                assert kids
                for k in kids:
                    assert (qlo[c, k] >= qlo[n, side]).all() and (qhi[c, k] <= qhi[n, side]).all(), (n, side, c, k)
    assert checked == int(live.sum())


@pytest.mark.parametrize("name,step", STEPS, ids=STEP_IDS)
def test_walk_of_the_refitted_tree_equals_the_scan(hpt, oracle_mod, name, step):
    L, sp, tr = rc.records(name, step)
    scan, s_scan = rc.scan(oracle_mod, name, step)
    walk, s_walk = oracle_mod.pt_render(L, sp, tr, rc.camera(name), rc.W, rc.H, rc.DEPTH, rc.SPP, seed=rc.SEED, bvh=rc.tree(hpt, name, step))
    print("%s step %d: boxes per closest ray %.1f" % (name, step, s_walk["boxes_closest"] / 2 / max(s_walk["closest_rays"], 1)))
    assert np.array_equal(walk, scan)
    assert all(s_walk[k] == s_scan[k] for k in RAYS)


# ---- the table ---------------------------------------------------------------------------------------------------------

def test_the_table_has_the_cases_the_suite_is_about():
    assert rc.NAMES == ["identity", "turn", "out", "shrink", "scramble", "die-and-return", "coincide", "there-and-back", "tiny-1", "tiny-2",
                        "tiny-3", "rounds", "parallel"]
    assert [len(rc.data(n).tr) for n in ("tiny-1", "tiny-2", "tiny-3")] == [1, 2, 3]
    assert len(rc.data("scramble").tr) == 3012
    for (name, step), n in rc.N_DEAD.items():
        assert int(rc.dead(rc.records(name, step)[2]).sum()) == n, (name, step)
    for name, step in STEPS:
        d, (L, sp, tr) = rc.data(name), rc.records(name, step)
        assert len(tr) == len(d.tr) and len(L) == len(d.L) and len(sp) == len(d.sp)
        # an update moves vertices (and round primitives) only
        for f in ("mtl_old", "mtl", "id"):
            assert tr[f].tobytes() == d.tr[f].tobytes(), (name, step, f)
    assert rc.is_rounds_step("rounds", 0) and not rc.is_rounds_step("rounds", 1) and rc.is_triangle_step("rounds", 1)
    assert sum(rc.is_rounds_step(n, s) for n, s in STEPS) == 1


def test_the_scrambled_tree_is_deep_and_irregular(hpt):
    assert rc.tree(hpt, "scramble", -1)["bvh_depth"] >= 12


@pytest.mark.parametrize("name,step", STEPS, ids=STEP_IDS)
def test_every_step_changes_the_image(oracle_mod, name, step):
    """... in 5 % of the pixels at least, so that a device structure left stale by an update cannot render the step's bytes."""
    now, before = rc.scan(oracle_mod, name, step)[0], rc.scan(oracle_mod, name, step - 1)[0]
    share = rc.changed_share(now, before)
    print("%s step %d: %.1f %% of the pixels change, %.1f %% lit" % (name, step, 100 * share, 100 * bc.lit_share(now)))
    assert np.isfinite(now).all() and now.any()
    if (name, step) in rc.SAME_AS_BEFORE:
        assert share == 0.0
    else:
        assert share >= 0.05


def test_the_sphere_moved_out_is_lit(oracle_mod):
    """Primary rays through the pixel centres: those whose closest hit is a triangle of the moved sphere -- which lies
    wholly outside the base scene's grid -- are many, and lit."""
    d, (L, sp, tr) = rc.data("out"), rc.records("out", 0)
    v_old, v_new = rc.verts(d.tr).reshape(-1, 3), rc.verts(tr)[rc.NWALL - 2:].reshape(-1, 3)
    assert v_new[:, 2].max() < v_old[:, 2].min()                                # beyond the old scene box
    cam = rc.camera("out")
    eye, ul, dx, dy = (np.asarray(cam[k], np.float64).reshape(3) for k in ("eye", "UL", "dx", "dy"))
    ys, xs = np.mgrid[0:rc.H, 0:rc.W]
    p = ul + dx * (xs[..., None] + 0.5) + dy * (ys[..., None] + 0.5)
    rd = p - eye
    rd = (rd / np.linalg.norm(rd, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32)
    ro = np.broadcast_to(eye.astype(np.float32), rd.shape).copy()
    _, prim = oracle_mod.closest_hits(L, sp, tr, ro, rd)
    on_sphere = (prim.reshape(rc.H, rc.W) >= len(L) + len(sp) + rc.NWALL - 2)
    img = rc.scan(oracle_mod, "out", 0)[0]
    lit = (img != 0).any(axis=-1)
    print("out: %d pixels on the moved sphere, %d of them lit" % (on_sphere.sum(), (on_sphere & lit).sum()))
    assert on_sphere.sum() >= 0.05 * rc.W * rc.H and (on_sphere & lit).sum() >= 0.5 * on_sphere.sum()


def test_the_photon_mapping_step_depends_on_the_bounds(tmp_path):
    """The oracle's image of PPM_STEP's records under the base scene's bounds differs from the one under the new bounds:
    a handle that kept its old bounds after the update would fail the GPU half."""
    lib = ppm_oracle.build(tmp_path)
    name, step = rc.PPM_STEP
    d, (L, sp, tr) = rc.data(name), rc.records(name, step)
    kw = dict(rc.PPM)
    args = (lib, L, sp, tr, rc.camera(name), rc.W, rc.H, kw["eye_depth"], kw["light_depth"], kw["spp"], kw["spl"], kw["radius"])
    new, st = ppm_oracle.render(*args, seed=kw["seed"])
    old_min, old_max = ppm_oracle.scene_bounds(d.sp, d.tr)
    old, _ = ppm_oracle.render(*args, seed=kw["seed"], scene_min=old_min, scene_max=old_max)
    assert st["deposits"] > 100 and rc.changed_share(new, old) >= 0.05


# ---- the refusals, without a device -----------------------------------------------------------------------------------------

def _refused(hpt, call, *words):
    with pytest.raises(hpt.HptError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith("hpt error 1:"), msg
    for w in words:
        assert w in msg, msg


def test_refusals_without_a_device(hpt):
    """hpt_scene_update_check on a null scene; the checks it shares with hpt_bvh_refit_host through that entry point (a
    scene handle cannot exist without a device: the count mismatch against a live handle, the other device and the
    handle left as it was are the GPU half's)."""
    d = rc.data("tiny-3")
    _refused(hpt, lambda: hpt.update_check(None, d.tr), "null scene")
    _refused(hpt, lambda: hpt.update_check(None, None, 0), "null scene")
    _refused(hpt, lambda: hpt.refit_bvh_host(d.L, d.sp, d.tr, d.tr[:2]), "count")
    for field, sub, value in (("mtl", "roughness", 0.5), ("mtl", "eta", 1.5), ("mtl_old", "Kd", 0.25), ("id", None, 77)):
        bad = d.tr.copy()
        if sub is None:
            bad[field][1] = value
        else:
            col = bad[field][sub].copy(); col[1] = value; bad[field][sub] = col
        assert rc.verts(bad).tobytes() == rc.verts(d.tr).tobytes()
        _refused(hpt, lambda: hpt.refit_bvh_host(d.L, d.sp, d.tr, bad), "triangle 1")
    lib = hpt.load_library()
    info = hpt.BvhInfo()
    tr = np.ascontiguousarray(d.tr)
    rc_ = lib.hpt_bvh_refit_host(None, 0, None, 0, tr.ctypes.data_as(C.c_void_p), None, len(tr), C.byref(info), None, C.c_size_t(0), None, C.c_size_t(0))
    assert rc_ == 1 and b"null" in lib.hpt_last_error()
    rc_ = lib.hpt_scene_update_check(None, tr.ctypes.data_as(C.c_void_p), len(tr))
    assert rc_ == 1 and b"null scene" in lib.hpt_last_error()
    # a scene of zero triangles takes an update of zero triangles
    empty = hpt.refit_bvh_host(d.L, d.sp, d.tr[:0], d.tr[:0])
    same_tree(empty, hpt.export_bvh_host(d.L, d.sp, d.tr[:0]))


# ---- undefined behaviour: the refit alone, under the sanitizers --------------------------------------------------------

SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def refit_check(tmp_path_factory):
    """tests/refit_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in, compiled the way
    test_build_cases_cpu.py compiles build_check.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("refit_check") / "refit_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "refit_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    return exe


def _fnv(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("name", rc.NAMES)
def test_refit_is_clean_under_the_sanitizers(hpt, refit_check, tmp_path, name):
    """The program refits step after step on ONE HostScene; every step's tree is the one refit_bvh_host gives from the base
    scene directly: a refit is a function of the topology and the new vertices alone, whatever the vertices before."""
    d = rc.data(name)
    steps = [s for s in range(len(d.steps)) if rc.is_triangle_step(name, s)]
    rec = str(tmp_path / "records.bin")
    L, sp, tr = (np.ascontiguousarray(a) for a in (d.L, d.sp, d.tr))
    assert (L.dtype.itemsize, sp.dtype.itemsize, tr.dtype.itemsize) == (144, 100, 120)
    with open(rec, "wb") as f:
        f.write(np.array([len(L), len(sp), len(tr), len(steps)], np.int32).tobytes())
        f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())
        for s in steps:
            f.write(np.ascontiguousarray(rc.records(name, s)[2]).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([refit_check, rec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    lines = [dict(kv.split("=") for kv in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert [int(o["step"]) for o in lines] == [-1] + list(range(len(steps)))
    for o, s in zip(lines, [-1] + steps):
        bvh = rc.tree(hpt, name, s)
        assert (int(o["nodes"]), int(o["tris"]), int(o["depth"])) == (bvh["num_nodes"], bvh["num_tris"], bvh["bvh_depth"]), s
        assert int(o["qnodes_fnv"], 16) == _fnv(bvh["qnodes"].tobytes()) and int(o["tris_fnv"], 16) == _fnv(bvh["tris"].tobytes()), s
        assert int(o["grid_fnv"], 16) == _fnv(bvh["qscale"].tobytes(), _fnv(bvh["qorigin"].tobytes())), s
        if s >= 0:
            assert int(o["dead"]) == int(rc.dead(rc.records(name, s)[2]).sum()), s
    # the four-wide tree's boxes follow the same chain: back at the base vertices they are the build's
    back = [i for i, s in enumerate(steps) if rc.records(name, s)[2].tobytes() == d.tr.tobytes()]
    for i in back:
        assert lines[i + 1]["wnodes_fnv"] == lines[0]["wnodes_fnv"]


# ---- the same bytes whatever the CPU count --------------------------------------------------------------------------------

def _big():
    """99 024 triangles (the benchmark's tree): the host's O(n) passes run on several threads from 65 536 elements on."""
    from path_tracing_amd import scene_io as sio
    L, sp, tr = sio.cornell_with_sphere(100000)
    ball = slice(rc.NWALL, None)
    return L, sp, tr, rc.with_verts(tr, rc.rotate_z(rc.rotate_y(rc.verts(tr)[ball], rc.SPHERE_C, 30.0), rc.SPHERE_C, 30.0), ball)


def _child(k):
    """In a process of its own (the library reads the CPU count once per process): pinned to the first k CPUs, prints a
    digest of the refitted tree."""
    cpus = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, cpus[:k])
    import path_tracing_amd as hpt
    L, sp, tr, tr2 = _big()
    bvh = hpt.refit_bvh_host(L, sp, tr, tr2)
    print("DIGEST " + json.dumps({key: hashlib.sha1(np.ascontiguousarray(bvh[key]).tobytes()).hexdigest() for key in TREE_KEYS}))


def test_refitted_tree_is_the_same_bytes_on_one_cpu_and_on_all():
    avail = len(os.sched_getaffinity(0))
    assert avail >= 2, "needs a process that may use two CPUs at least"
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_refit_cpu as t\nt._child(int(sys.argv[1]))\n" % (ROOT, HERE)
    procs = [subprocess.Popen([sys.executable, "-c", code, str(k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in (1, avail)]
    out = []
    for p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, se[-2000:]
        out.append(json.loads([ln for ln in so.splitlines() if ln.startswith("DIGEST ")][-1][7:]))
    assert out[0] == out[1]
