"""The device build's definition on the host (include/hpt.h, "device builds"; csrc/scene_build.cpp, lbvh_host_scene), on every
case of device_build_cases.py: its topology against the Python restatement of lbvh_oracle.py, the tree's well-formedness, the
oracle's walk of it against the scan, refits of it, the same bytes on any number of CPUs, a clean run under the sanitizers,
and the refusals that need no device.  No GPU."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import device_build_cases as dc
import lbvh_oracle as lo
from test_bvh_walk import _check_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
BYTE_KEYS = ("qnodes", "tris", "qorigin", "qscale", "num_nodes", "num_tris", "bvh_depth", "num_rounds")
TOPOLOGY_WORDS = ((("qnodes"), (6, 7)), (("tris"), (3, 7, 11)))       # child codes; ordinal, material, flags


def same_tree(got, want, keys=BYTE_KEYS):
    for k in keys:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), k


def test_constants_are_the_headers(hpt):
    with open(os.path.join(CSRC, "hpt_scene.h")) as f:
        text = f.read()
    assert int(re.search(r"constexpr int kMaxLeafTris = (\d+);", text).group(1)) == dc.MAX_LEAF_TRIS == lo.MAX_LEAF_TRIS
    assert int(re.search(r"constexpr int kMaxBvhDepth = (\d+);", text).group(1)) == dc.MAX_BVH_DEPTH
    assert C.sizeof(hpt.DeviceBuildInfo) == 64 and C.sizeof(hpt.RebuildInfo) == 48


# ---- the Python restatement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.NAMES)
def test_topology_is_the_python_restatement(hpt, name):
    L, sp, tr = dc.records(name)
    bvh = dc.tree(hpt, name)
    want = lo.build(tr, len(sp) + len(L))
    assert bvh["num_rounds"] == len(sp) + len(L) and bvh["num_tris"] == len(tr)
    assert bvh["num_nodes"] == len(want["left"])
    assert np.array_equal(bvh["qnodes"][:, 6], want["left"]) and np.array_equal(bvh["qnodes"][:, 7], want["right"])
    assert np.array_equal(bvh["tris"][:, 3], want["ordinals"])
    assert bvh["bvh_depth"] == want["depth"] == bvh["build"]["depth_after"]
    assert bvh["build"]["nodes_after"] == bvh["num_nodes"] and bvh["build"]["builds"] == 1
    assert bvh["build"]["fell_back"] == (1 if name in dc.FALLS_BACK else 0)


def test_deep63_is_a_chain_of_powers_of_two(hpt):
    L, sp, tr = dc.records("deep63")
    key = lo.keys(tr)
    assert sorted(key[2:]) == [1 << b for b in range(63)]
    cell, _ = lo.cells(tr)
    assert [tuple(c) for c in cell[2:].tolist()] == dc.deep63_cells()
    bvh = dc.tree(hpt, "deep63")
    print("deep63: %d levels, wide_depth %d" % (bvh["bvh_depth"], bvh["build"]["wide_depth"]))
    assert bvh["bvh_depth"] > dc.MAX_BVH_DEPTH and bvh["build"]["fell_back"] == 1


def test_equal_keys_and_dead_keys(hpt):
    assert len(set(lo.keys(dc.records("equal-64")[2]))) == 1
    for name, n in dc.N_DEAD.items():
        assert lo.keys(dc.records(name)[2]).count(lo.DEAD_KEY) == n == int(lo.dead(dc.records(name)[2]).sum())
    cell, _ = lo.cells(dc.records("planar")[2])
    assert (cell[:, 2] == 0).all() and len(set(map(tuple, cell.tolist()))) > 50


# ---- well-formedness -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.NAMES)
def test_tree_is_well_formed(hpt, name):
    L, sp, tr = dc.records(name)
    bvh = dc.tree(hpt, name)
    nt, nn = len(tr), bvh["num_nodes"]
    _check_tree(bvh, nt)                               # every triangle in one leaf slot, every node reached once from the root
    qn = bvh["qnodes"]
    # every node of depth d precedes every node of depth d + 1, and the levels add up
    depth = np.full(nn, -1, np.int64)
    depth[0] = 0
    for i in range(nn):
        assert depth[i] >= 0
        for c in (int(qn[i, 6]), int(qn[i, 7])):
            if not c & 0x80000000:
                assert c > i and depth[c] < 0
                depth[c] = depth[i] + 1
    assert (np.diff(depth) >= 0).all()
    level_begin = lo.build(tr, bvh["num_rounds"])["level_begin"]
    counts = np.bincount(depth)
    assert level_begin[0] == 0 and level_begin[-1] == nn and np.array_equal(np.diff(level_begin), counts)
    assert bvh["bvh_depth"] == (len(counts) if nt else 0)
    cost = hpt.tree_cost_host(bvh)
    assert cost["leaf_slots"] == nt and cost["inner_children"] + 1 == nn
    # a leaf holds kMaxLeafTris triangles at most
    codes = np.concatenate([qn[:, 6], qn[:, 7]])
    leaves = codes[(codes != 0xFFFFFFFF) & ((codes & 0x80000000) != 0)]
    assert ((leaves & 7) + 1 <= dc.MAX_LEAF_TRIS).all()


# ---- the host walk -------------------------------------------------------------------------------------------------------

WALKED = [n for n in dc.NAMES if n not in dc.FALLS_BACK]         # (the device never walks a tree it fell back from)


@pytest.mark.parametrize("name", WALKED)
def test_oracle_through_the_tree_equals_the_scan(hpt, oracle_mod, name):
    L, sp, tr = dc.records(name)
    bvh = dc.tree(hpt, name)
    kw = dict(seed=dc.SEED)
    if name in dc.BIG:
        kw["window"] = (8, 6, 24, 18)
    scan, s_scan = oracle_mod.pt_render(L, sp, tr, dc.camera(), dc.W, dc.H, dc.DEPTH, dc.SPP, **kw)
    walk, s_walk = oracle_mod.pt_render(L, sp, tr, dc.camera(), dc.W, dc.H, dc.DEPTH, dc.SPP, bvh=bvh, **kw)
    assert np.array_equal(scan, walk)
    assert all(s_walk[k] == s_scan[k] for k in ("closest_rays", "shadow_rays"))
    print("%s: %d triangles, nodes %d, depth %d, boxes per closest ray %.1f (3 log2 N = %.1f)"
          % (name, len(tr), bvh["num_nodes"], bvh["bvh_depth"], s_walk["boxes_closest"] / 2 / max(s_walk["closest_rays"], 1), 3 * np.log2(max(len(tr), 2))))


# ---- refits --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", dc.SMALL)
def test_refit_of_the_build(hpt, name):
    L, sp, tr = dc.records(name)
    bvh = dc.tree(hpt, name)
    same_tree(hpt.device_build_bvh_host(L, sp, tr, tr), bvh)          # to its own records: the plain build's bytes
    new = dc.moved(tr)
    moved = hpt.device_build_bvh_host(L, sp, tr, new)
    for key, words in TOPOLOGY_WORDS:
        for w in words:
            assert np.array_equal(moved[key][:, w], bvh[key][:, w]), (key, w)
    assert moved["bvh_depth"] == bvh["bvh_depth"] and moved["num_nodes"] == bvh["num_nodes"]
    if len(tr) > 12 and not lo.dead(tr).all():
        assert moved["tris"].tobytes() != bvh["tris"].tobytes()
    # the leaf records are the new vertices'
    idx = moved["tris"][:, 3].astype(np.int64) - moved["num_rounds"]
    assert np.array_equal(moved["tris"][:, 0:3].view(np.float32).view(np.uint32), np.ascontiguousarray(new["v0"][idx]).view(np.uint32))
    cost = hpt.tree_cost_host(moved)
    assert cost["leaf_slots"] == len(tr)


# ---- the same bytes on any number of CPUs --------------------------------------------------------------------------------

THREAD_CASES = ["grid-stride", "scramble", "build:nan-20-middle"]


def _child(k, names):
    """Runs in a process of its own (the library reads the CPU count once per process): pins itself to the first k of the CPUs
    it was given, builds, prints one JSON line of digests."""
    cpus = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, cpus[:k])
    assert len(os.sched_getaffinity(0)) == k
    import path_tracing_amd as hpt
    out = {}
    for name in names:
        bvh = hpt.device_build_bvh_host(*dc.records(name))
        out[name] = {key: hashlib.sha1(np.ascontiguousarray(bvh[key]).tobytes()).hexdigest() for key in BYTE_KEYS}
    print("DIGESTS " + json.dumps(out))


def test_tree_does_not_depend_on_the_cpu_count():
    avail = len(os.sched_getaffinity(0))
    ks = sorted({k for k in (1, 2, avail) if k <= avail})
    assert len(ks) >= 2, "needs a process that may use two CPUs at least"
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_device_build_cpu as t\nt._child(int(sys.argv[1]), sys.argv[2:])\n" % (ROOT, HERE)
    procs = {k: subprocess.Popen([sys.executable, "-c", code, str(k)] + THREAD_CASES, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in ks}
    out = {}
    for k, p in procs.items():
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, (k, se[-2000:])
        out[k] = json.loads([ln for ln in so.splitlines() if ln.startswith("DIGESTS ")][-1][8:])
    for k in ks[1:]:
        assert out[k] == out[ks[0]], "the tree differs between %d and %d CPUs" % (k, ks[0])


# ---- undefined behaviour: the definition alone, under the sanitizers -----------------------------------------------------

SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def lbvh_check(tmp_path_factory):
    """tests/lbvh_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in, compiled the way
    test_build_cases_cpu.py compiles build_check.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("lbvh_check") / "lbvh_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "lbvh_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    return exe


@pytest.mark.parametrize("name", dc.NAMES)
def test_definition_is_clean_under_the_sanitizers(hpt, lbvh_check, tmp_path, name):
    L, sp, tr = dc.records(name)
    rec, out_file = str(tmp_path / "records.bin"), str(tmp_path / "tree.bin")
    L, sp, tr = np.ascontiguousarray(L), np.ascontiguousarray(sp), np.ascontiguousarray(tr)
    with open(rec, "wb") as f:
        f.write(np.array([len(L), len(sp), len(tr)], np.int32).tobytes())
        f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([lbvh_check, rec, out_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    # the program writes what it built: the library's tree
    said = dict(kv.split("=") for kv in p.stdout.decode().split())
    bvh = dc.tree(hpt, name)
    assert (int(said["nodes"]), int(said["tris"]), int(said["depth"]), int(said["wide_depth"])) == \
           (bvh["num_nodes"], bvh["num_tris"], bvh["bvh_depth"], bvh["build"]["wide_depth"])
    with open(out_file, "rb") as f:
        assert f.read() == bvh["qnodes"].tobytes() + bvh["tris"].tobytes()


# ---- refusals that need no device ----------------------------------------------------------------------------------------

def test_refusals(hpt):
    lib = hpt.load_library()
    L, sp, tr = dc.records("tiny-5")
    info, binfo = hpt.BvhInfo(), hpt.DeviceBuildInfo()
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    zero = C.c_size_t(0)

    def refused(rc_, word):
        assert rc_ == 1 and word in lib.hpt_last_error(), lib.hpt_last_error()
    refused(lib.hpt_scene_rebuild_device(None), b"null scene")
    refused(lib.hpt_scene_get_device_build_info(None, C.byref(binfo)), b"null")
    refused(lib.hpt_bvh_device_build_host(vp(L), len(L), vp(sp), len(sp), vp(tr), None, len(tr), None, C.byref(binfo), None, zero, None, zero), b"null info")
    refused(lib.hpt_bvh_device_build_host(vp(L), len(L), vp(sp), len(sp), vp(tr), None, -1, C.byref(info), C.byref(binfo), None, zero, None, zero), b"negative")
    refused(lib.hpt_bvh_device_build_host(vp(L), len(L), vp(sp), len(sp), None, None, len(tr), C.byref(info), C.byref(binfo), None, zero, None, zero), b"null primitive")
    bad = tr.copy()
    bad["mtl"]["roughness"][3] = 0.25
    refused(lib.hpt_bvh_device_build_host(vp(L), len(L), vp(sp), len(sp), vp(tr), vp(bad), len(tr), C.byref(info), C.byref(binfo), None, zero, None, zero),
            b"triangle 3")
    small = np.zeros(4, np.uint32)
    refused(lib.hpt_bvh_device_build_host(vp(L), len(L), vp(sp), len(sp), vp(tr), None, len(tr), C.byref(info), C.byref(binfo), vp(small), C.c_size_t(16), None, zero),
            b"qnodes_out too small")
    with pytest.raises(hpt.HptError):
        hpt.device_build_bvh_host(L, sp, tr, tr[:4])
    # ... and what is right is accepted, with a null binfo too
    assert lib.hpt_bvh_device_build_host(vp(L), len(L), vp(sp), len(sp), vp(tr), None, len(tr), C.byref(info), None, None, zero, None, zero) == 0
    assert (info.num_nodes, info.num_tris, info.bvh_depth) == (2, 5, 2)
