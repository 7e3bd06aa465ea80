"""Skinning on the host alone (skin_cases.py): hpt_skin_host, the definition, held to the numpy restatement of
skin_oracle.py byte for byte on every skin step; the rigid case held to hpt_pose_host and the keep case to its input; the
skinned records through hpt_bvh_refit_host to well-formed trees of the base tree's topology whose walk gives the scan's
image; the table held to its own conditions (every step changes the image, so a structure left stale cannot pass the GPU
half, tests/test_gpu_skin.py; `bend` holds corners that a fused multiply-add would round differently in a row and others
in the blend sum, so a kernel compiled with contraction cannot pass it either; all three cases, inactive and non-finite
bones and dead triangles are reached); the refusals that need no handle; and the chains of skins of die-and-return and
bones-3001 in a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_cases as pc
import pose_oracle as po
import refit_cases as rc
import skin_cases as sc
import skin_oracle as so
from test_bvh_walk import _check_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
TREE_KEYS = ("num_nodes", "num_tris", "bvh_depth", "num_rounds", "qorigin", "qscale", "qnodes", "tris")
SKINS = sc.skin_steps()
SKIN_IDS = ["%s-%d" % s for s in SKINS]
SCANNED = [n for n in sc.NAMES if n != "grid-stride"]               # (grid-stride is rendered by the walk alone: see skin_cases)
GEOMETRY = sc.all_geometry_steps(SCANNED)
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

@pytest.mark.parametrize("name,step", SKINS, ids=SKIN_IDS)
def test_skin_host_equals_the_oracle(hpt, name, step):
    d = sc.data(name)
    want, rest, (_, bone, weight) = sc.expected(name)[step]
    got = hpt.skin_host(rest, bone, weight, d.steps[step][1])
    _same_bytes("%s step %d" % (name, step), got, want)
    for f in ("mtl_old", "mtl", "id"):                               # only vertices move
        assert got[f].tobytes() == d.tr[f].tobytes(), f


def test_a_one_hot_skin_is_a_pose_byte_for_byte(hpt):
    d, p = sc.data("rigid"), pc.data("turn")
    _, bone, weight, _ = d.steps[0]
    assert (np.ascontiguousarray(weight).view(U32) != 0).sum(axis=-1).max() == 1 and set(np.unique(weight)) == {0.0, 1.0}
    for step in (1, 2, 3):
        posed = hpt.pose_host(p.tr, p.steps[0][1], p.steps[step][1])
        _same_bytes("rigid step %d against hpt_pose_host" % step, hpt.skin_host(d.tr, bone, weight, d.steps[step][1]), posed)
        assert sc.records("rigid", step)[2].tobytes() == pc.records("turn", step)[2].tobytes()


def test_keep_returns_the_inputs_bytes(hpt):
    d = sc.data("keep")
    _, bone, weight, _ = d.steps[0]
    bits = po.verts_of(d.tr).view(U32)
    assert bits[0, 1, 0] == 0x80000000 and bits[11, 2, 1] == 0x7FC12345
    for step in (1, 2):
        assert hpt.skin_host(d.tr, bone, weight, d.steps[step][1]).tobytes() == d.tr.tobytes(), step
    assert np.isnan(d.steps[2][1][2]).all()                        # ... whatever the weightless bone holds
    got = po.verts_of(hpt.skin_host(d.tr, bone, weight, d.steps[3][1])).view(U32)
    assert np.array_equal(got[:sc.NWALL], bits[:sc.NWALL])          # the walls keep -0 and the payload while the sphere blends
    assert not np.array_equal(got[sc.NWALL:], bits[sc.NWALL:])
    # identity records under two weights are kept, but the same weights on an identity in value only (-0.0) are arithmetic
    almost = pc.identity(3); almost[1, 0, 1] = -0.0
    got = po.verts_of(hpt.skin_host(d.tr, bone, weight, almost)).view(U32)
    want = so.skin_verts(po.verts_of(d.tr), bone, weight, almost).view(U32)
    assert np.array_equal(got, want) and (so.cases(bone, weight, almost)[sc.NWALL:] == so.BLEND).all()
    assert not np.array_equal(got[sc.NWALL:], bits[sc.NWALL:])          # 0.3 x + 0.7 x is not x for every x
    assert sc.records("die-and-return", 4)[2].tobytes() == sc.data("die-and-return").tr.tobytes()      # all back is the base


# ---- every step: the tree of the skinned records ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,step", GEOMETRY, ids=GEOMETRY_IDS)
def test_skinned_records_refit_to_a_well_formed_tree_that_renders_the_scan(hpt, oracle_mod, name, step):
    base, bvh = sc.tree(hpt, name, -1), sc.tree(hpt, name, step)
    L, sp, tr = sc.records(name, step)
    _check_tree(bvh, len(tr))
    for k in ("num_nodes", "num_tris", "bvh_depth", "num_rounds"):
        assert bvh[k] == base[k], k
    assert np.array_equal(bvh["qnodes"][:, 6:8], base["qnodes"][:, 6:8])                    # the base tree's codes
    assert np.array_equal(bvh["tris"][:, [3, 7, 11]], base["tris"][:, [3, 7, 11]])
    assert np.isfinite(bvh["qorigin"]).all() and np.isfinite(bvh["qscale"]).all() and (bvh["qscale"] > 0).all()
    scan, s_scan = sc.scan(oracle_mod, name, step)
    walk, s_walk = oracle_mod.pt_render(L, sp, tr, sc.camera(name), sc.W, sc.H, sc.DEPTH, sc.SPP, seed=sc.SEED, bvh=bvh)
    assert np.array_equal(walk, scan)
    assert all(s_walk[k] == s_scan[k] for k in ("closest_rays", "shadow_rays"))


def test_the_grid_stride_case_refits_to_a_well_formed_tree(hpt):
    bvh = sc.tree(hpt, "grid-stride", 1)
    _check_tree(bvh, sc.N_STRIDE)
    assert bvh["num_nodes"] == sc.tree(hpt, "grid-stride", -1)["num_nodes"]


# ---- the table ---------------------------------------------------------------------------------------------------------

def test_the_table_has_the_cases_the_suite_is_about():
    assert sc.NAMES == ["rigid", "keep", "bend", "four", "die-and-return", "rest-rule", "swap", "tiny-1", "tiny-2", "tiny-3",
                        "edges-85", "edges-86", "edges-171", "edges-256", "grid-stride",
                        "bones-1", "bones-256", "bones-257", "bones-3001", "bones-65536"]
    assert [len(sc.data(n).tr) for n in ("tiny-1", "tiny-2", "tiny-3", "edges-85", "edges-86", "edges-171", "edges-256", "bend")] == [1, 2, 3, 85, 86, 171, 256, 276]
    assert [(3 * n) % 256 for n in sc.EDGE_COUNTS] == [255, 2, 1, 0]         # one lane per corner, workgroups of 256
    # the first count whose corners exceed the capped grid
    assert len(sc.data("grid-stride").tr) == sc.N_STRIDE and 3 * sc.N_STRIDE == 2048 * 256 + 1 and 3 * (sc.N_STRIDE - 1) <= 2048 * 256
    for nb in sc.BONE_COUNTS:                                      # every table's last bone is named, with weight and without
        _, bone, weight, num_bones = sc.data("bones-%d" % nb).steps[0]
        assert num_bones == nb and bone.max() == nb - 1 and bone.min() == 0
        assert (weight[bone == nb - 1] > 0).any() and (weight[bone == nb - 1] == 0).any()
    assert sc.BONE_COUNTS == (1, 256, 257, 3001, 65536)
    assert [s[0] for s in sc.data("rest-rule").steps] == ["set", "skin", "tris", "skin", "dverts", "skin"]
    assert [s[0] for s in sc.data("swap").steps] == ["set", "skin", "parts", "pose", "set", "skin"]
    for (name, step), n in sc.N_DEAD.items():
        assert int(rc.dead(sc.records(name, step)[2]).sum()) == n, (name, step)
    w = sc.data("four").steps[0][2][sc.NWALL:]
    assert ((w.view(U32) != 0).sum(axis=-1) == 4).all() and set(np.unique(w.sum(axis=-1))) == {0.5, 2.0}
    for name in sc.NAMES:
        d = sc.data(name)
        for step in range(len(d.steps)):
            tr = sc.records(name, step)[2]
            assert len(tr) == len(d.tr)
            for f in ("mtl_old", "mtl", "id"):
                assert tr[f].tobytes() == d.tr[f].tobytes(), (name, step, f)


def test_the_table_reaches_every_case_inactive_and_non_finite_bones_and_dead_triangles():
    seen = np.zeros(3, np.int64)
    for name, step in SKINS:
        _, _, (_, bone, weight) = sc.expected(name)[step]
        seen += np.bincount(so.cases(bone, weight, sc.data(name).steps[step][1]).reshape(-1), minlength=3)
    print("corners kept, rigid, blended over the table:", seen.tolist())
    assert (seen > 0).all()
    # bend alone reaches all three: the foot is kept, the top rigid by a weight of 1.0f, the rest blends
    _, bone, weight, _ = sc.data("bend").steps[0]
    assert (np.bincount(so.cases(bone, weight, sc.data("bend").steps[1][1]).reshape(-1), minlength=3) > 0).all()
    # die-and-return, step 1: non-finite records that are named without weight (no effect) and with weight (dead)
    d = sc.data("die-and-return")
    _, bone, weight, _ = d.steps[0]
    xf = d.steps[1][1]
    bad_bone = ~np.isfinite(xf).all(axis=(1, 2))
    assert bad_bone.tolist() == [False, False, True, True, False]
    named, active = bad_bone[bone], weight.view(U32) != 0
    idle = (named & ~active).any(axis=(1, 2)) & ~(named & active).any(axis=(1, 2))
    hit = (named & active).any(axis=(1, 2))
    dead = rc.dead(sc.records("die-and-return", 1)[2])
    assert idle.sum() == 612 and hit.sum() == 400 and not dead[idle].any() and dead[hit].all() and dead.sum() == 400
    # step 3: every record finite, a weight of 1e30 overflows
    assert np.isfinite(d.steps[3][1]).all() and weight.max() == np.float32(1e30)
    assert rc.dead(sc.records("die-and-return", 3)[2]).sum() == 100 and rc.dead(sc.records("die-and-return", 2)[2]).sum() == 0


@pytest.mark.parametrize("name,step", sc.all_geometry_steps(), ids=["%s-%d" % s for s in sc.all_geometry_steps()])
def test_every_step_changes_the_image(hpt, oracle_mod, name, step):
    """... in 5 % of the pixels at least against the step before (the refit suite's own condition), so that a device
    structure left stale by a skin cannot render the step's bytes."""
    now, before = sc.scan(oracle_mod, name, step, hpt)[0], sc.scan(oracle_mod, name, step - 1, hpt)[0]
    share = rc.changed_share(now, before)
    print("%s step %d: %.1f %% of the pixels change" % (name, step, 100 * share))
    assert np.isfinite(now).all()
    if (name, step) in sc.SAME_AS_BEFORE:
        assert share == 0.0
    else:
        assert share >= 0.05


def test_bend_holds_corners_a_fused_multiply_add_rounds_differently():
    """Corners whose bits change when the rows alone are contracted, and corners whose bits change when the blend sum
    alone is: a kernel compiled with contraction in either place cannot reproduce the case."""
    d = sc.data("bend")
    _, bone, weight, _ = d.steps[0]
    v = po.verts_of(d.tr)
    rows_total = sum_total = 0
    for step in (1, 2, 3):
        xf = d.steps[step][1]
        blended = so.cases(bone, weight, xf) == so.BLEND
        plain = so.raw(v, bone, weight, xf).view(U32)
        in_rows = ((so.fused(v, bone, weight, xf, rows=True, blend=False).view(U32) != plain).any(axis=-1) & blended).sum()
        in_sum = ((so.fused(v, bone, weight, xf, rows=False, blend=True).view(U32) != plain).any(axis=-1) & blended).sum()
        print("bend step %d: corners whose fused form differs: %d in a row, %d in the blend sum, of %d blended" % (step, in_rows, in_sum, blended.sum()))
        rows_total += in_rows
        sum_total += in_sum
    assert rows_total > 0 and sum_total > 0


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
    bone = np.zeros((3, 3, 4), np.int32); bone[..., 1] = 1
    weight = np.full((3, 3, 4), 0.25, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.hpt_scene_set_skin(None, vp(bone), vp(weight), 3, 2) == 1 and b"null scene" in lib.hpt_last_error()
    assert lib.hpt_scene_skin(None, vp(rec), 2) == 1 and b"null scene" in lib.hpt_last_error()
    _refused(hpt, lambda: hpt.skin_host(tr, bone, weight, pc.identity(0).reshape(0, 3, 4)), "bones")
    assert lib.hpt_skin_host(vp(tr), 3, vp(bone), vp(weight), vp(rec), 65537, vp(out)) == 1 and b"bones" in lib.hpt_last_error()

    def edited(a, at, value):
        a = a.copy(); a[at] = value
        return a
    _refused(hpt, lambda: hpt.skin_host(tr, edited(bone, (1, 2, 3), 2), weight, rec), "triangle 1 corner 2")
    _refused(hpt, lambda: hpt.skin_host(tr, edited(bone, (2, 0, 0), -1), weight, rec), "triangle 2 corner 0")
    # ... active or not
    _refused(hpt, lambda: hpt.skin_host(tr, edited(bone, (0, 1, 2), 2), edited(weight, (0, 1, 2), 0.0), rec), "triangle 0 corner 1")
    for bad in (-0.0, -0.5, float("nan"), float("inf"), -float("inf")):
        _refused(hpt, lambda: hpt.skin_host(tr, bone, edited(weight, (2, 1, 0), bad), rec), "triangle 2 corner 1", "negative or not finite")
    # the first one in corner order is named
    _refused(hpt, lambda: hpt.skin_host(tr, edited(bone, (2, 2, 0), 9), edited(weight, (1, 0, 3), -1.0), rec), "triangle 1 corner 0")
    _refused(hpt, lambda: hpt.skin_host(tr, bone[:2], weight[:2], rec), "twelve influences per triangle")
    _refused(hpt, lambda: hpt.skin_host(tr, bone, weight[:2], rec), "four bones and four weights per corner")
    assert lib.hpt_skin_host(vp(tr), 3, None, vp(weight), vp(rec), 2, vp(out)) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_skin_host(vp(tr), 3, vp(bone), None, vp(rec), 2, vp(out)) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_skin_host(vp(tr), 3, vp(bone), vp(weight), None, 2, vp(out)) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_skin_host(None, 3, vp(bone), vp(weight), vp(rec), 2, vp(out)) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_skin_host(vp(tr), 3, vp(bone), vp(weight), vp(rec), 2, None) == 1 and b"null" in lib.hpt_last_error()
    assert lib.hpt_skin_host(vp(tr), -1, vp(bone), vp(weight), vp(rec), 2, vp(out)) == 1 and b"negative" in lib.hpt_last_error()
    assert out.tobytes() == tr.tobytes()                          # a refused call writes nothing
    # zero triangles with zero counts, and a skin in place
    assert lib.hpt_skin_host(None, 0, None, None, vp(rec), 2, None) == 0
    turn = pc.table(po.IDENTITY, pc.affine(pc.rot_y(10.0)))
    assert lib.hpt_skin_host(vp(out), 3, vp(bone), vp(weight), vp(turn), 2, vp(out)) == 0
    _same_bytes("in place", out, so.skin(tr, bone, weight, turn))


# ---- undefined behaviour: the chains of skins, under the sanitizers ------------------------------------------------

SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def skin_check(tmp_path_factory):
    """tests/skin_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in, compiled the way
    test_pose_cpu.py compiles pose_check.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("skin_check") / "skin_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "skin_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    return exe


def _fnv(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("name", ["die-and-return", "bones-3001"])
def test_the_chain_of_skins_is_clean_under_the_sanitizers(hpt, skin_check, tmp_path, name):
    """The program skins the base records step after step and refits ONE HostScene to each; every step's records are the
    oracle's and every tree the one hpt_bvh_refit_host gives from the base scene directly."""
    d = sc.data(name)
    kind, bone, weight, num_bones = d.steps[0]
    assert kind == "set"
    steps = [s for s in range(1, len(d.steps)) if d.steps[s][0] == "skin"]
    assert len(steps) == len(d.steps) - 1
    rec = str(tmp_path / "records.bin")
    L, sp, tr = (np.ascontiguousarray(a) for a in (d.L, d.sp, d.tr))
    with open(rec, "wb") as f:
        f.write(np.array([len(L), len(sp), len(tr), num_bones, len(steps)], np.int32).tobytes())
        f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())
        f.write(np.ascontiguousarray(bone, np.int32).tobytes())
        f.write(np.ascontiguousarray(weight, np.float32).tobytes())
        for s in steps:
            f.write(np.ascontiguousarray(d.steps[s][1], np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([skin_check, rec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    lines = [dict(kv.split("=") for kv in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert [int(o["step"]) for o in lines] == [-1] + list(range(len(steps)))
    for o, s in zip(lines, [-1] + steps):
        bvh, want = sc.tree(hpt, name, s), np.ascontiguousarray(sc.records(name, s)[2])
        assert int(o["records_fnv"], 16) == _fnv(want.tobytes()), s
        assert (int(o["nodes"]), int(o["tris"]), int(o["depth"])) == (bvh["num_nodes"], bvh["num_tris"], bvh["bvh_depth"]), s
        assert int(o["qnodes_fnv"], 16) == _fnv(bvh["qnodes"].tobytes()) and int(o["tris_fnv"], 16) == _fnv(bvh["tris"].tobytes()), s
        assert int(o["grid_fnv"], 16) == _fnv(bvh["qscale"].tobytes(), _fnv(bvh["qorigin"].tobytes())), s
        if s >= 0:
            assert int(o["dead"]) == int(rc.dead(want).sum()), s
