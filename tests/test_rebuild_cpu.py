"""The tree cost (include/hpt.h, "tree cost") on the host alone: hpt_bvh_cost_host against the numpy restatement
(cost_oracle.py) on the scenes of rebuild_cases.HOST_SCENES -- integers equal, doubles bit for bit --, the two identities
every tree obeys, the cost of a refitted tree against the cost of the tree the builder gives for the same records on every
step of refit_cases.py, the refusals, and the definition in a stand-alone program under the address and
undefined-behaviour sanitizers (host code only)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cost_oracle as co
import rebuild_cases as rb
import refit_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "path_tracing_amd", "csrc")
STEPS = rc.all_steps()
_BUILT = {}


def built(hpt, name, step):
    """The builder's tree for the records after `step` of a refit case (the tree a rebuild gives), once per process."""
    if (name, step) not in _BUILT:
        _BUILT[(name, step)] = hpt.export_bvh_host(*rc.records(name, step))
    return _BUILT[(name, step)]


def _identities(what, c, num_tris):
    """Every child is inner, a leaf or empty; every triangle sits in exactly one leaf slot, dead ones included (the builder
    keeps a dead triangle in a leaf at the dead point: it is tested, so it counts)."""
    assert c["inner_children"] + c["leaf_children"] + c["empty_children"] == 2 * c["num_nodes"], what
    assert c["leaf_slots"] == num_tris, what
    assert c["inner_children"] == c["num_nodes"] - 1, what          # every node but the root is some node's inner child


@pytest.mark.parametrize("name", rb.HOST_NAMES)
def test_host_cost_equals_the_restatement(hpt, name):
    L, sp, tr = rb.host_scene(name)
    bvh = hpt.export_bvh_host(L, sp, tr)
    got, want = hpt.tree_cost_host(bvh), co.cost(bvh)
    co.same(name, got, want)
    _identities(name, got, len(tr))
    assert got["num_nodes"] == bvh["num_nodes"] >= 1
    if name in rb.NON_FINITE_GRID:
        assert not np.isfinite(bvh["qscale"]).any()
        assert (got["box_visits"], got["tri_tests"], got["sah"]) == (0.0, 0.0, 0.0)
    elif len(tr) and not rc.dead(tr).all():
        assert got["box_visits"] >= 1.0 and got["tri_tests"] > 0.0 and got["sah"] == 2.0 * got["box_visits"] + got["tri_tests"]
    if name.startswith("tiny-"):
        n = int(name[5:])
        # a leaf holds up to two triangles, so two triangles are one leaf beside an empty child, as one is
        assert got["empty_children"] == (2, 1, 1, 0)[n] and got["leaf_slots"] == n and got["num_nodes"] == 1, got
        if n == 0:
            assert got["root_extent"] == (0, 0, 0) and got["sah"] == 0.0
    if name.startswith("nodes-"):
        assert bvh["num_nodes"] == int(name[6:]) and len(tr) == rb.NODE_EDGES[bvh["num_nodes"]]


def test_the_case_table_names_what_it_says():
    assert set(rb.NON_FINITE_GRID) < set(rb.HOST_NAMES) and len(rb.NON_FINITE_GRID) >= 1
    assert all("build:" + c.name in rb.HOST_SCENES for c in rb.bc.CASES)
    assert [len(rb.host_scene("tiny-%d" % n)[2]) for n in range(4)] == [0, 1, 2, 3]
    for name in rb.STATE_NAMES:
        st = rb.state(name)
        assert len(st.calls) >= 1 and len(st.base[2]) >= 264


@pytest.mark.parametrize("name,step", STEPS)
def test_refitted_against_rebuilt_on_every_step(hpt, name, step):
    """Both trees hold the same records; both costs equal the restatement; the identity step gives equal structs."""
    tr = rc.records(name, step)[2]
    refit, rebuilt = rc.tree(hpt, name, step), built(hpt, name, step)
    c_refit, c_rebuilt = hpt.tree_cost_host(refit), hpt.tree_cost_host(rebuilt)
    co.same("%s step %d, refitted" % (name, step), c_refit, co.cost(refit))
    co.same("%s step %d, rebuilt" % (name, step), c_rebuilt, co.cost(rebuilt))
    _identities((name, step, "refitted"), c_refit, len(tr))
    _identities((name, step, "rebuilt"), c_rebuilt, len(tr))
    print("%s step %d: sah refitted %.4f, rebuilt %.4f" % (name, step, c_refit["sah"], c_rebuilt["sah"]))
    if (name, step) == ("identity", 0):
        assert c_refit["bytes"] == c_rebuilt["bytes"]
        co.same("identity: refitted against rebuilt", c_refit, c_rebuilt)


def test_scramble_costs_more_refitted_than_rebuilt(hpt, oracle_mod):
    """The project's unkind case.  Only the strict inequality is asserted; the ratio, and beside it the ratio of the host
    walk's boxes per closest-hit ray on the same two trees (the oracle's walk), are printed for DESIGN.md, "Rebuilds"."""
    name = "scramble"
    for step in range(len(rc.data(name).steps)):
        L, sp, tr = rc.records(name, step)
        refit, rebuilt = rc.tree(hpt, name, step), built(hpt, name, step)
        c_refit, c_rebuilt = hpt.tree_cost_host(refit), hpt.tree_cost_host(rebuilt)
        boxes = []
        for bvh in (refit, rebuilt):
            _, st = oracle_mod.pt_render(L, sp, tr, rc.camera(name), rc.W, rc.H, rc.DEPTH, rc.SPP, seed=rc.SEED, bvh=bvh)
            boxes.append(st["boxes_closest"] / 2 / max(st["closest_rays"], 1))
        print("scramble step %d: sah refitted %.2f, rebuilt %.2f, ratio %.2f; box_visits %.2f / %.2f; boxes per closest ray (host walk) %.1f / %.1f, ratio %.2f"
              % (step, c_refit["sah"], c_rebuilt["sah"], c_refit["sah"] / c_rebuilt["sah"], c_refit["box_visits"], c_rebuilt["box_visits"],
                 boxes[0], boxes[1], boxes[0] / boxes[1]))
        assert c_refit["sah"] > c_rebuilt["sah"]


def test_refusals_of_the_host_cost(hpt):
    lib = hpt.load_library()
    L, sp, tr = rb.host_scene("tiny-3")
    bvh = hpt.export_bvh_host(L, sp, tr)
    qn = np.ascontiguousarray(bvh["qnodes"], np.uint32)
    vp = qn.ctypes.data_as(C.c_void_p)
    info = hpt.BvhInfo(bvh["num_nodes"], bvh["num_tris"], bvh["bvh_depth"], bvh["num_rounds"])
    for a in range(3):
        info.qscale[a] = bvh["qscale"][a]
    out = hpt.TreeCost()
    full = C.c_size_t(qn.nbytes)

    def refused(rc_, word):
        assert rc_ == 1 and word in lib.hpt_last_error(), lib.hpt_last_error()
    refused(lib.hpt_bvh_cost_host(None, vp, full, C.byref(out)), b"null")
    refused(lib.hpt_bvh_cost_host(C.byref(info), None, full, C.byref(out)), b"null")
    refused(lib.hpt_bvh_cost_host(C.byref(info), vp, full, None), b"null")
    refused(lib.hpt_bvh_cost_host(C.byref(info), vp, C.c_size_t(qn.nbytes - 1), C.byref(out)), b"num_nodes * 32")
    for bad in (0, -1):
        refused(lib.hpt_bvh_cost_host(C.byref(hpt.BvhInfo(bad, 0, 0, 0)), vp, full, C.byref(out)), b"at least one node")
    refused(lib.hpt_bvh_cost_host(C.byref(hpt.BvhInfo(1 << 24, 0, 0, 0)), vp, C.c_size_t(32 << 24), C.byref(out)), b"2^24")
    assert lib.hpt_bvh_cost_host(C.byref(info), vp, full, C.byref(out)) == 0          # ... and what is right is accepted
    assert bytes(out) == co.pack(co.cost(bvh))
    # the scene-side refusals that need no scene
    refused(lib.hpt_scene_tree_cost(None, C.byref(out)), b"null")
    refused(lib.hpt_scene_rebuild(None), b"null scene")
    refused(lib.hpt_scene_get_rebuild_info(None, None), b"null")


# ---- undefined behaviour: the definition alone, under the sanitizers -----------------------------------------------------

SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]
SAN_SCENES = [n for n in rb.HOST_NAMES] + ["refit:" + n for n in rc.NAMES]


@pytest.fixture(scope="module")
def cost_check(tmp_path_factory):
    """tests/cost_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in, compiled the way
    test_build_cases_cpu.py compiles build_check.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("cost_check") / "cost_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "cost_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    return exe


@pytest.mark.parametrize("name", SAN_SCENES)
def test_cost_is_clean_under_the_sanitizers(hpt, cost_check, tmp_path, name):
    """The program prints what it computed: the library's struct, field for field, for the builder's tree and -- on the refit
    cases -- for the tree refitted to every triangle step."""
    if name.startswith("refit:"):
        case = name[6:]
        d = rc.data(case)
        L, sp, tr = d.L, d.sp, d.tr
        steps = [s for s in range(len(d.steps)) if rc.is_triangle_step(case, s)]
        moved = [rc.records(case, s)[2] for s in steps]
        trees = [rc.tree(hpt, case, -1)] + [rc.tree(hpt, case, s) for s in steps]
    else:
        L, sp, tr = rb.host_scene(name)
        moved, trees = [], [hpt.export_bvh_host(L, sp, tr)]
    L, sp, tr = (np.ascontiguousarray(a) for a in (L, sp, tr))
    assert (L.dtype.itemsize, sp.dtype.itemsize, tr.dtype.itemsize) == (144, 100, 120)
    rec = str(tmp_path / "records.bin")
    with open(rec, "wb") as f:
        f.write(np.array([len(L), len(sp), len(tr), len(moved)], np.int32).tobytes())
        f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())
        for m in moved:
            f.write(np.ascontiguousarray(m).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([cost_check, rec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    lines = [dict(kv.split("=") for kv in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert [int(o["step"]) for o in lines] == list(range(-1, len(moved)))
    for o, bvh in zip(lines, trees):
        want = hpt.tree_cost_host(bvh)
        got = {k: int(o[k]) for k in co.INT_KEYS + ("num_nodes",)}
        got["root_extent"] = (int(o["rx"]), int(o["ry"]), int(o["rz"]))
        for k in co.DOUBLE_KEYS:
            got[k] = np.array([int(o[k], 16)], np.uint64).view(np.float64)[0].item()
        co.same("%s step %s" % (name, o["step"]), got, want)
