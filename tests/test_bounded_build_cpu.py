"""The bounded device build's definition on the host (include/hpt.h, "bounded device builds"; csrc/scene_build.cpp,
lbvh_bounded_host_scene) on every pair of bounded_cases.py: its topology and counts against the Python restatement of
bounded_oracle.py, the depth bound, the unbounded definition's bytes where nothing was forced, well-formedness, the oracle's
walk of the tree against the scan, refits, the refusals that need no device, and a stand-alone program under the sanitizers.
No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bounded_cases as bcs
import bounded_oracle as bo
import device_build_cases as dc
import lbvh_oracle as lo
from test_bvh_walk import _check_tree
from test_device_build_cpu import BYTE_KEYS, SAN_FLAGS, TOPOLOGY_WORDS, WALKED, same_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
INFO_KEYS = ("max_depth", "forced_nodes", "first_forced_level")
PAIR_ARGS = dict(argnames="pair", argvalues=bcs.ALL_PAIRS, ids=[bcs.pair_id(p) for p in bcs.ALL_PAIRS])


def test_constants_and_the_table(hpt):
    assert C.sizeof(hpt.BoundedBuildInfo) == 16 and C.sizeof(hpt.DeviceBuildInfo) == 64
    assert bo.MAX_BVH_DEPTH == dc.MAX_BVH_DEPTH
    assert [bo.need(n) for n in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 1 << 20, (1 << 20) + 1)] == [1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 19, 20]
    assert bcs.need_of("grid-stride") == bcs.BIG_NEED
    for name in dc.SMALL:
        if name == "deep63":
            continue
        n = bcs.need_of(name)
        want = {0, 1} if name.startswith("tiny-") and n == 1 else {0, n} if name.startswith("tiny-") else {0, n, n + 1, (n + 30) // 2}
        assert {d for m, d in bcs.PAIRS if m == name} == want, name
    for name, d in bcs.ALL_PAIRS:
        assert bo.effective_depth(len(bcs.records(name)[2]), d) is not None, (name, d)
    for name, d in bcs.REFUSED:
        assert bo.effective_depth(len(bcs.records(name)[2]), d) is None, (name, d)


# ---- the Python restatement, the bound, the unbounded tree -----------------------------------------------------------------

@pytest.mark.parametrize(**PAIR_ARGS)
def test_topology_is_the_python_restatement(hpt, pair):
    name, depth = pair
    L, sp, tr = bcs.records(name)
    bvh = bcs.tree(hpt, name, depth)
    want = bo.build(tr, len(sp) + len(L), depth)
    assert bvh["num_rounds"] == len(sp) + len(L) and bvh["num_tris"] == len(tr)
    assert bvh["num_nodes"] == len(want["left"])
    assert np.array_equal(bvh["qnodes"][:, 6], want["left"]) and np.array_equal(bvh["qnodes"][:, 7], want["right"])
    assert np.array_equal(bvh["tris"][:, 3], want["ordinals"])
    assert bvh["bvh_depth"] == want["depth"] == bvh["build"]["depth_after"]
    assert bvh["bounded"] == {k: want[k] for k in INFO_KEYS}
    D = depth or dc.MAX_BVH_DEPTH
    assert bvh["bounded"]["max_depth"] == D and bvh["bvh_depth"] <= D
    assert bvh["build"]["nodes_after"] == bvh["num_nodes"] and bvh["build"]["builds"] == 1
    assert bvh["build"]["wide_depth"] <= max(bvh["bvh_depth"], 1)
    assert bvh["build"]["fell_back"] == (1 if bvh["build"]["wide_depth"] > 19 else 0)
    if depth == bcs.need_of(name) and len(tr) > 4:
        # the root is forced, and every left child below it down its spine (a right child may need fewer levels than are left)
        assert bvh["bounded"]["first_forced_level"] == 0 and bvh["bounded"]["forced_nodes"] >= bvh["bvh_depth"] == depth


def test_unforced_builds_are_the_unbounded_definition(hpt):
    """Both branches are taken: some pairs force nothing and give lbvh_host_scene's bytes, some force nodes and do not."""
    unforced, forced = [], []
    for name, depth in bcs.ALL_PAIRS:
        bvh = bcs.tree(hpt, name, depth)
        if bvh["bounded"]["forced_nodes"]:
            assert bvh["bounded"]["first_forced_level"] < bvh["bvh_depth"]
            forced.append((name, depth))
            continue
        assert bvh["bounded"]["first_forced_level"] == bo.NONE_FORCED
        plain = dc.tree(hpt, name) if name in dc.CASES else hpt.device_build_bvh_host(*bcs.records(name))
        same_tree(bvh, plain)
        assert {k: bvh["build"][k] for k in ("nodes_after", "depth_after", "wide_depth")} == {k: plain["build"][k] for k in ("nodes_after", "depth_after", "wide_depth")}
        unforced.append((name, depth))
    print("%d pairs with nothing forced, %d with forced nodes" % (len(unforced), len(forced)))
    assert len(unforced) >= 1 and len(forced) >= 1
    assert ("deep63", 0) in forced and ("grid-stride", 0) in unforced


def test_deep63_fits_where_the_radix_tree_does_not(hpt):
    plain = dc.tree(hpt, "deep63")
    assert plain["bvh_depth"] == 61 and plain["build"]["fell_back"] == 1
    for depth, levels in ((0, 30), (7, 7), (6, 6)):
        bvh = bcs.tree(hpt, "deep63", depth)
        print("deep63 at %d: %d levels, wide_depth %d, %s" % (depth, bvh["bvh_depth"], bvh["build"]["wide_depth"], bvh["bounded"]))
        assert bvh["bvh_depth"] <= levels and bvh["build"]["fell_back"] == 0 and bvh["bounded"]["forced_nodes"] > 0


# ---- well-formedness -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize(**PAIR_ARGS)
def test_tree_is_well_formed(hpt, pair):
    name, depth = pair
    L, sp, tr = bcs.records(name)
    bvh = bcs.tree(hpt, name, depth)
    nt, nn = len(tr), bvh["num_nodes"]
    _check_tree(bvh, nt)                               # every triangle in one leaf slot, every node reached once from the root
    cost = hpt.tree_cost_host(bvh)
    assert cost["leaf_slots"] == nt and cost["inner_children"] + 1 == nn
    qn = bvh["qnodes"]
    codes = np.concatenate([qn[:, 6], qn[:, 7]])
    inner = codes[(codes & 0x80000000) == 0]
    assert np.array_equal(np.sort(inner), np.arange(1, nn))          # breadth-first numbers: each once
    assert (np.diff(qn[:, 6][(qn[:, 6] & 0x80000000) == 0].astype(np.int64)) > 0).all()
    leaves = codes[(codes != 0xFFFFFFFF) & ((codes & 0x80000000) != 0)]
    assert ((leaves & 7) + 1 <= dc.MAX_LEAF_TRIS).all()


# ---- the host walk -------------------------------------------------------------------------------------------------------

WALKED_PAIRS = [p for p in bcs.ALL_PAIRS if p[0] in WALKED or p[0] in ("deep63", "edge-2049")]


@pytest.mark.parametrize("pair", WALKED_PAIRS, ids=[bcs.pair_id(p) for p in WALKED_PAIRS])
def test_oracle_through_the_tree_equals_the_scan(hpt, oracle_mod, scans, pair):
    name, depth = pair
    L, sp, tr = bcs.records(name)
    bvh = bcs.tree(hpt, name, depth)
    kw = dict(seed=dc.SEED)
    if name in dc.BIG:
        kw["window"] = (8, 6, 24, 18)
    if name not in scans:
        scans[name] = oracle_mod.pt_render(L, sp, tr, dc.camera(), dc.W, dc.H, dc.DEPTH, dc.SPP, **kw)
    scan, s_scan = scans[name]
    walk, s_walk = oracle_mod.pt_render(L, sp, tr, dc.camera(), dc.W, dc.H, dc.DEPTH, dc.SPP, bvh=bvh, **kw)
    assert np.array_equal(scan, walk)
    assert all(s_walk[k] == s_scan[k] for k in ("closest_rays", "shadow_rays"))


@pytest.fixture(scope="module")
def scans():
    """The scan's render of a case, once for all its depths."""
    return {}


# ---- refits --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pair", bcs.PAIRS, ids=[bcs.pair_id(p) for p in bcs.PAIRS])
def test_refit_of_the_build(hpt, pair):
    name, depth = pair
    L, sp, tr = bcs.records(name)
    bvh = bcs.tree(hpt, name, depth)
    same_tree(hpt.device_build_bounded_bvh_host(L, sp, tr, tr, depth), bvh)          # to its own records: the plain build's bytes
    new = dc.moved(tr)
    moved = hpt.device_build_bounded_bvh_host(L, sp, tr, new, depth)
    for key, words in TOPOLOGY_WORDS:
        for w in words:
            assert np.array_equal(moved[key][:, w], bvh[key][:, w]), (key, w)
    assert moved["bvh_depth"] == bvh["bvh_depth"] and moved["num_nodes"] == bvh["num_nodes"] and moved["bounded"] == bvh["bounded"]
    if len(tr) > 12 and not lo.dead(tr).all():
        assert moved["tris"].tobytes() != bvh["tris"].tobytes()
    idx = moved["tris"][:, 3].astype(np.int64) - moved["num_rounds"]
    assert np.array_equal(moved["tris"][:, 0:3].view(np.float32).view(np.uint32), np.ascontiguousarray(new["v0"][idx]).view(np.uint32))
    assert hpt.tree_cost_host(moved)["leaf_slots"] == len(tr)
    if bvh["bounded"]["forced_nodes"] == 0:
        same_tree(moved, hpt.device_build_bvh_host(L, sp, tr, new))


# ---- refusals that need no device ----------------------------------------------------------------------------------------

def test_refusals(hpt):
    lib = hpt.load_library()
    L, sp, tr = bcs.records("tiny-5")
    info, binfo, bb = hpt.BvhInfo(), hpt.DeviceBuildInfo(), hpt.BoundedBuildInfo()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    zero = C.c_size_t(0)

    def refused(rc_, word):
        assert rc_ == 1 and word in lib.hpt_last_error(), lib.hpt_last_error()

    def host(tris, new, nt, info_, depth, qn=None, qcap=zero):
        return lib.hpt_bvh_device_build_bounded_host(vp(L), len(L), vp(sp), len(sp), tris, new, nt, info_, C.byref(binfo), qn, qcap, None, zero,
                                                     C.c_int(depth), C.byref(bb))
    refused(lib.hpt_scene_rebuild_device_bounded(None, C.c_int(0)), b"null scene")
    refused(lib.hpt_scene_get_bounded_build_info(None, C.byref(bb)), b"null")
    refused(host(vp(tr), None, len(tr), None, 0), b"null info")
    refused(host(vp(tr), None, -1, C.byref(info), 0), b"negative")
    refused(host(None, None, len(tr), C.byref(info), 0), b"null primitive")
    for depth in (-1, 31, 1, -2147483648, 2147483647):              # five triangles need two levels
        refused(host(vp(tr), None, len(tr), C.byref(info), depth), b"max_depth")
    bad = tr.copy()
    bad["mtl"]["roughness"][3] = 0.25
    refused(host(vp(tr), vp(bad), len(tr), C.byref(info), 0), b"triangle 3")
    small = np.zeros(4, np.uint32)
    refused(host(vp(tr), None, len(tr), C.byref(info), 0, vp(small), C.c_size_t(16)), b"qnodes_out too small")
    with pytest.raises(hpt.HptError):
        hpt.device_build_bounded_bvh_host(L, sp, tr, tr[:4])
    for name, depth in bcs.REFUSED:
        with pytest.raises(hpt.HptError) as e:
            hpt.device_build_bounded_bvh_host(*bcs.records(name), None, depth)
        assert str(e.value).startswith("hpt error 1:") and "max_depth" in str(e.value)
    # ... and what is right is accepted, with null records to fill too
    assert lib.hpt_bvh_device_build_bounded_host(vp(L), len(L), vp(sp), len(sp), vp(tr), None, len(tr), C.byref(info), None, None, zero, None, zero,
                                                 C.c_int(2), None) == 0
    assert (info.num_nodes, info.num_tris, info.bvh_depth) == (2, 5, 2)
    assert host(vp(tr), None, len(tr), C.byref(info), 2) == 0 and (bb.max_depth, bb.forced_nodes, bb.first_forced_level) == (2, 2, 0)     # the root and its child of four


# ---- undefined behaviour: the definition alone, under the sanitizers -----------------------------------------------------

def test_definition_is_clean_under_the_sanitizers(tmp_path):
    """tests/bounded_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in, compiled the way
    test_device_build_cpu.py compiles lbvh_check.cpp, run as a child process."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path / "bounded_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "bounded_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-1500:] + p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    lines = p.stdout.decode().splitlines()
    assert lines[-1] == "bad=0" and len(lines) == 41
    said = [dict(kv.split("=") for kv in ln.split()) for ln in lines[:-1]]
    assert any(int(s["unbounded_depth"]) > 30 and int(s["depth_at_0"]) <= 30 and int(s["forced_at_0"]) > 0 for s in said)      # the deep scenes are deep
    assert any(int(s["forced_at_0"]) == 0 and int(s["n"]) >= 1000 for s in said)
