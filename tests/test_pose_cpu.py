"""Poses on the host alone (pose_cases.py): hpt_pose_host, the definition, held to the numpy restatement of
pose_oracle.py byte for byte on every pose step; the posed records through hpt_bvh_refit_host to well-formed trees of the
base tree's topology whose walk gives the scan's image; the table held to its own conditions (every step changes the
image, so a structure left stale cannot pass the GPU half, tests/test_gpu_pose.py; `turn` holds vertices that a fused
multiply-add would round differently, so a kernel compiled with contraction cannot pass it either); the two rules on
bits; the refusals that need no handle; and the chains of poses of die-and-return and per-triangle in a stand-alone
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_cases as pc
import pose_oracle as po
import refit_cases as rc
from test_bvh_walk import _check_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
TREE_KEYS = ("num_nodes", "num_tris", "bvh_depth", "num_rounds", "qorigin", "qscale", "qnodes", "tris")
POSES = pc.pose_steps()
POSE_IDS = ["%s-%d" % s for s in POSES]
GEOMETRY = pc.all_geometry_steps(pc.POSE_NAMES)                  # (the dv- cases replay refit_cases' steps, which its own suite holds)
GEOMETRY_IDS = ["%s-%d" % s for s in GEOMETRY]
U32 = np.uint32


def _same_bytes(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        a, b = po.verts_of(got).view(U32), po.verts_of(want).view(U32)
        at = np.argwhere(a != b)
        pytest.fail("%s: %d vertex words differ, first at %s: got %08x, expected %08x" % (what, len(at), at[0].tolist(), a[tuple(at[0])], b[tuple(at[0])]))


# ---- the definition against its restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,step", POSES, ids=POSE_IDS)
def test_pose_host_equals_the_oracle(hpt, name, step):
    d = pc.data(name)
    want, rest, part = pc.expected(name)[step]
    got = hpt.pose_host(rest, part, d.steps[step][1])
    _same_bytes("%s step %d" % (name, step), got, want)
    # only vertices move
    for f in ("mtl_old", "mtl", "id"):
        assert got[f].tobytes() == d.tr[f].tobytes(), f


def test_a_null_part_map_is_one_part(hpt):
    _, _, tr = pc.base()
    rec = pc.table(pc.affine(pc.tilted(20.0), rc.SPHERE_C))
    _same_bytes("one part", hpt.pose_host(tr, None, rec), po.pose(tr, None, rec))


# ---- every step: the tree of the posed records ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,step", GEOMETRY, ids=GEOMETRY_IDS)
def test_posed_records_refit_to_a_well_formed_tree_that_renders_the_scan(hpt, oracle_mod, name, step):
    base, bvh = pc.tree(hpt, name, -1), pc.tree(hpt, name, step)
    L, sp, tr = pc.records(name, step)
    _check_tree(bvh, len(tr))
    for k in ("num_nodes", "num_tris", "bvh_depth", "num_rounds"):
        assert bvh[k] == base[k], k
    assert np.array_equal(bvh["qnodes"][:, 6:8], base["qnodes"][:, 6:8])                    # the base tree's codes
    assert np.array_equal(bvh["tris"][:, [3, 7, 11]], base["tris"][:, [3, 7, 11]])
    assert np.isfinite(bvh["qorigin"]).all() and np.isfinite(bvh["qscale"]).all() and (bvh["qscale"] > 0).all()
    scan, s_scan = pc.scan(oracle_mod, name, step)
    walk, s_walk = oracle_mod.pt_render(L, sp, tr, pc.camera(name), pc.W, pc.H, pc.DEPTH, pc.SPP, seed=pc.SEED, bvh=bvh)
    assert np.array_equal(walk, scan)
    assert all(s_walk[k] == s_scan[k] for k in ("closest_rays", "shadow_rays"))


def test_identity_keeps_the_builders_tree_and_the_inputs_bytes(hpt):
    d = pc.data("identity")
    for k in TREE_KEYS:
        a, b = np.ascontiguousarray(pc.tree(hpt, "identity", 1)[k]), np.ascontiguousarray(pc.tree(hpt, "identity", -1)[k])
        assert a.tobytes() == b.tobytes(), k
    assert pc.records("identity", 1)[2].tobytes() == d.tr.tobytes()
    assert pc.records("die-and-return", 6)[2].tobytes() == pc.data("die-and-return").tr.tobytes()      # ... and all back is the base


# ---- the table ---------------------------------------------------------------------------------------------------------

def test_the_table_has_the_cases_the_suite_is_about():
    assert pc.NAMES == ["identity", "turn", "out", "shrink", "shear-mirror", "die-and-return", "per-triangle", "tiny-1", "tiny-2", "tiny-3",
                        "edges-85", "edges-171", "edges-256", "interleave", "dv-turn", "dv-die-and-return", "dv-tiny-1", "dv-tiny-2", "dv-tiny-3"]
    assert [len(pc.data(n).tr) for n in ("tiny-1", "tiny-2", "tiny-3", "edges-85", "edges-171", "edges-256")] == [1, 2, 3, 85, 171, 256]
    # one lane per vertex, workgroups of 256: one lane short, one lane over, exactly full
    assert [(3 * n) % 256 for n in pc.EDGE_COUNTS] == [255, 1, 0]
    d = pc.data("per-triangle")
    kind, part, num_parts = d.steps[0]
    assert kind == "parts" and num_parts == 3001 and len(d.tr) == 3012 and num_parts > 256       # past the table the kernel stages in LDS
    owned = np.bincount(part, minlength=num_parts)
    assert owned[0] == 12 and (owned[1:2999] == 1).all() and owned[2999] == 2 and owned[3000] == 0
    assert [s[0] for s in pc.data("interleave").steps] == ["parts", "pose", "tris", "pose", "dverts", "pose", "parts", "pose"]
    for (name, step), n in pc.N_DEAD.items():
        assert int(rc.dead(pc.records(name, step)[2]).sum()) == n, (name, step)
    for name in pc.NAMES:
        d = pc.data(name)
        for step in range(len(d.steps)):
            tr = pc.records(name, step)[2]
            assert len(tr) == len(d.tr)
            for f in ("mtl_old", "mtl", "id"):
                assert tr[f].tobytes() == d.tr[f].tobytes(), (name, step, f)
    # the device-vertex cases are refit_cases' steps, record for record
    for src in pc.DV_SOURCES:
        for step in range(len(rc.data(src).steps)):
            assert pc.records("dv-" + src, step)[2].tobytes() == rc.records(src, step)[2].tobytes(), (src, step)


@pytest.mark.parametrize("name,step", GEOMETRY, ids=GEOMETRY_IDS)
def test_every_step_changes_the_image(oracle_mod, name, step):
    """... in 5 % of the pixels at least against the step before (the refit suite's own condition), so that a device
    structure left stale by a pose cannot render the step's bytes."""
    now, before = pc.scan(oracle_mod, name, step)[0], pc.scan(oracle_mod, name, step - 1)[0]
    share = rc.changed_share(now, before)
    print("%s step %d: %.1f %% of the pixels change" % (name, step, 100 * share))
    assert np.isfinite(now).all()
    if (name, step) in pc.SAME_AS_BEFORE:
        assert share == 0.0
    else:
        assert share >= 0.05


def test_turn_holds_vertices_a_fused_multiply_add_rounds_differently():
    """At least one vertex per axis whose fused evaluation (emulated in float64) has other bits than the definition's,
    in the 30-degree step alone: a kernel compiled with contraction cannot reproduce it.  (At 60 and 90 degrees some
    entries of the record are exact -- 0.5, 1 -- and their products with them: those rows fuse to the same bits.)"""
    d = pc.data("turn")
    total = np.zeros(3, np.int64)
    for step in (1, 2, 3):
        _, rest, part = pc.expected("turn")[step]
        v = po.verts_of(rest)
        a, b = po.raw(v, part, d.steps[step][1]).view(U32), po.fused(v, part, d.steps[step][1]).view(U32)
        differ = (a != b)[part == 1].reshape(-1, 3).sum(axis=0)
        print("turn step %d: vertices whose fused form differs, per axis: %s" % (step, differ.tolist()))
        total += differ
        assert step != 1 or (differ >= 1).all(), (step, differ)
    assert (total >= 1).all()


# ---- the two rules on bits --------------------------------------------------------------------------------------------

def _odd_records():
    tr = pc.base()[2][:4].copy()
    v = po.verts_of(tr).view(U32).copy()
    v[0, 0, 0] = 0x80000000              # -0.0
    v[0, 1, 1] = 0x7FC12345              # a quiet NaN with a payload
    v[1, 2, 2] = 0xFFA00001              # a negative signalling NaN
    v[1, 0, 0] = 0x00000001              # the smallest denormal
    v[2, 0, 1] = 0x7F800000              # +inf
    return po.with_verts(tr, v.view(np.float32)), v


def test_identity_keeps_minus_zero_and_nan_payloads(hpt):
    tr, bits = _odd_records()
    got = hpt.pose_host(tr, np.array([0, 0, 0, 1], np.int32), pc.table(po.IDENTITY, pc.affine(np.eye(3), shift=(0.0, 0.0, 0.0))))
    assert np.array_equal(po.verts_of(got).view(U32)[:3], bits[:3])
    # a record that is the identity in value but not in bytes (-0.0 entries) is arithmetic: -0.0 becomes +0.0, NaN canonical
    almost = po.IDENTITY.copy(); almost[0, 1] = -0.0
    assert not po.is_identity(almost)[0]
    got = po.verts_of(hpt.pose_host(tr, None, almost[None])).view(U32)
    assert got[0, 0, 0] == 0x00000000
    assert (got[0, 1] == 0x7FC00000).all() and (got[1, 2] == 0x7FC00000).all() and (got[2, 0] == 0x7FC00000).all()
    assert got[1, 0, 0] == 0x00000001                              # denormals are kept, not flushed
    assert np.array_equal(got, po.pose_verts(po.verts_of(tr), np.zeros(4, np.int64), almost[None]).view(U32))


def test_a_result_that_is_not_finite_is_three_canonical_nans(hpt):
    _, _, tr = pc.base()
    d = pc.data("die-and-return")
    for step in (1, 3, 4, 5):
        want, rest, part = pc.expected("die-and-return")[step]
        raw = po.raw(po.verts_of(rest), part, d.steps[step][1])
        bad = ~np.isfinite(raw).all(axis=-1)
        assert bad.any()
        got = po.verts_of(hpt.pose_host(rest, part, d.steps[step][1])).view(U32)
        assert (got[bad] == 0x7FC00000).all()
        assert np.isfinite(got.view(np.float32)[~bad]).all()
    # step 4 reaches it by arithmetic: no NaN and no infinity in the table, every Z of part 1 overflows
    assert np.isfinite(d.steps[4][1]).all()
    _, rest, part = pc.expected("die-and-return")[4]
    raw = po.raw(po.verts_of(rest), part, d.steps[4][1])
    assert np.isposinf(raw[part == 1][..., 2]).all() and np.isfinite(raw[part == 1][..., :2]).all()


# ---- the refusals that need no handle --------------------------------------------------------------------------------

def _refused(hpt, call, *words):
    with pytest.raises(hpt.HptError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith("hpt error 1:"), msg
    for w in words:
        assert w in msg, msg


def test_refusals_without_a_device(hpt):
    lib = hpt.load_library()
    d = rc.data("tiny-3")
    tr = np.ascontiguousarray(d.tr)
    out = tr.copy()
    rec = pc.identity(2)
    part = np.array([0, 1, 1], np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for fn, args in (("hpt_scene_update_vertices_device", (None, None, 0)), ("hpt_scene_set_parts", (None, None, 0, 1)),
                     ("hpt_scene_pose", (None, vp(rec), 2)), ("hpt_scene_read_triangles", (None, None, 0))):
        assert getattr(lib, fn)(*args) == 1 and b"null scene" in lib.hpt_last_error(), fn
    _refused(hpt, lambda: hpt.pose_host(tr, part, pc.identity(0).reshape(0, 3, 4)), "parts")
    _refused(hpt, lambda: hpt.pose_host(tr, np.array([0, 2, 1], np.int32), rec), "triangle 1")
    _refused(hpt, lambda: hpt.pose_host(tr, np.array([0, 1, -1], np.int32), rec), "triangle 2")
    _refused(hpt, lambda: hpt.pose_host(tr, None, rec), "null part map")
    _refused(hpt, lambda: hpt.pose_host(tr, part[:2], rec), "one part index per triangle")
    assert lib.hpt_pose_host(vp(tr), 3, vp(part), vp(rec), (1 << 20) + 1, vp(out)) == 1 and b"parts" in lib.hpt_last_error()
    assert lib.hpt_pose_host(vp(tr), 3, vp(part), None, 2, vp(out)) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_pose_host(None, 3, vp(part), vp(rec), 2, vp(out)) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_pose_host(vp(tr), 3, vp(part), vp(rec), 2, None) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_pose_host(vp(tr), -1, vp(part), vp(rec), 2, vp(out)) == 1 and b"negative" in lib.hpt_last_error()
    assert out.tobytes() == tr.tobytes()                          # a refused call writes nothing
    # zero triangles with zero counts, and a pose in place
    assert lib.hpt_pose_host(None, 0, None, vp(rec), 2, None) == 0
    assert lib.hpt_pose_host(vp(out), 3, vp(part), vp(pc.table(po.IDENTITY, pc.affine(pc.rot_y(10.0)))), 2, vp(out)) == 0
    _same_bytes("in place", out, po.pose(tr, part, pc.table(po.IDENTITY, pc.affine(pc.rot_y(10.0)))))


# ---- undefined behaviour: the chains of poses, under the sanitizers ------------------------------------------------

SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def pose_check(tmp_path_factory):
    """tests/pose_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in, compiled the way
    test_refit_cpu.py compiles refit_check.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("pose_check") / "pose_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "pose_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    return exe


def _fnv(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("name", ["die-and-return", "per-triangle"])
def test_the_chain_of_poses_is_clean_under_the_sanitizers(hpt, pose_check, tmp_path, name):
    """The program poses the base records step after step and refits ONE HostScene to each; every step's records are the
    oracle's and every tree the one hpt_bvh_refit_host gives from the base scene directly."""
    d = pc.data(name)
    kind, part, num_parts = d.steps[0]
    assert kind == "parts"
    steps = [s for s in range(1, len(d.steps)) if d.steps[s][0] == "pose"]
    assert len(steps) == len(d.steps) - 1
    rec = str(tmp_path / "records.bin")
    L, sp, tr = (np.ascontiguousarray(a) for a in (d.L, d.sp, d.tr))
    with open(rec, "wb") as f:
        f.write(np.array([len(L), len(sp), len(tr), num_parts, len(steps)], np.int32).tobytes())
        f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())
        f.write(np.ascontiguousarray(part, np.int32).tobytes())
        for s in steps:
            f.write(np.ascontiguousarray(d.steps[s][1], np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([pose_check, rec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    lines = [dict(kv.split("=") for kv in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert [int(o["step"]) for o in lines] == [-1] + list(range(len(steps)))
    for o, s in zip(lines, [-1] + steps):
        bvh, want = pc.tree(hpt, name, s), np.ascontiguousarray(pc.records(name, s)[2])
        assert int(o["records_fnv"], 16) == _fnv(want.tobytes()), s
        assert (int(o["nodes"]), int(o["tris"]), int(o["depth"])) == (bvh["num_nodes"], bvh["num_tris"], bvh["bvh_depth"]), s
        assert int(o["qnodes_fnv"], 16) == _fnv(bvh["qnodes"].tobytes()) and int(o["tris_fnv"], 16) == _fnv(bvh["tris"].tobytes()), s
        assert int(o["grid_fnv"], 16) == _fnv(bvh["qscale"].tobytes(), _fnv(bvh["qorigin"].tobytes())), s
        if s >= 0:
            assert int(o["dead"]) == int(rc.dead(want).sum()), s
