"""The tree builder's threaded paths on the host (csrc/scene_build.cpp): the exported tree is a function of the input
alone -- the same bytes however many CPUs the building process may use -- and the paths that only large scenes take
(subtree threads above 8 192 triangles, parallel_chunks from 65 536, the big nodes' stable partition from 131 072)
build trees that are well formed and that return the scan's image."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_bvh_walk import _check_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE_KEYS = ("qnodes", "tris", "qorigin", "qscale", "num_nodes", "bvh_depth")
SCENES = ["sphere-140000", "sphere-300000", "random-70000", "sphere-20000"]


def _scene(sio, name):
    kind, n = name.split("-")
    return sio.cornell_with_sphere(int(n)) if kind == "sphere" else sio.cornell_random_triangles(int(n))


def leaf_sets(bvh):
    """The ordinals of every leaf in ascending order, leaves in slot order: what is left of `tris` when the order inside a
    leaf is taken away."""
    qn = bvh["qnodes"]
    codes = np.concatenate([qn[:, 6], qn[:, 7]])
    codes = codes[(codes != 0xFFFFFFFF) & ((codes & 0x80000000) != 0)]
    first, cnt = ((codes & 0x7FFFFFFF) >> 3).astype(np.int64), (codes & 7).astype(np.int64) + 1
    order = np.argsort(first)
    first, cnt = first[order], cnt[order]
    assert cnt.sum() == bvh["num_tris"] and np.array_equal(first, np.cumsum(cnt) - cnt)
    leaf_of_slot = np.repeat(np.arange(len(first)), cnt)
    ords = bvh["tris"][:, 3].astype(np.int64)
    return np.concatenate([first, cnt, ords[np.lexsort((ords, leaf_of_slot))]])


def digests(bvh):
    d = {k: hashlib.sha1(np.ascontiguousarray(bvh[k]).tobytes()).hexdigest() for k in BYTE_KEYS}
    d["leaf_sets"] = hashlib.sha1(leaf_sets(bvh).tobytes()).hexdigest()
    d["size"] = [int(bvh["num_nodes"]), int(bvh["num_tris"]), int(bvh["bvh_depth"])]
    return d


def _child(k, names):
    """Runs in a process of its own (the builder reads the CPU count once per process): pins itself to the first k of the
    CPUs it was given, builds, prints one JSON line of digests."""
    cpus = sorted(os.sched_getaffinity(0))
    os.sched_setaffinity(0, cpus[:k])
    assert len(os.sched_getaffinity(0)) == k
    import path_tracing_amd as hpt
    from path_tracing_amd import scene_io as sio
    out = {name: digests(hpt.export_bvh_host(*_scene(sio, name))) for name in names}
    print("DIGESTS " + json.dumps(out))


@pytest.fixture(scope="module")
def per_cpu_count():
    """{k: {scene: digests}} for k = 1, 2, 4 and every CPU this process may use (each k once)."""
    avail = len(os.sched_getaffinity(0))
    ks = sorted({k for k in (1, 2, 4, avail) if k <= avail})
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_build_threads_cpu as t\nt._child(int(sys.argv[1]), sys.argv[2:])\n" % (ROOT, os.path.join(ROOT, "tests"))
    procs = {k: subprocess.Popen([sys.executable, "-c", code, str(k)] + SCENES, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k in ks}
    out = {}
    for k, p in procs.items():
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, (k, se[-2000:])
        out[k] = json.loads([ln for ln in so.splitlines() if ln.startswith("DIGESTS ")][-1][8:])
    return out


def test_enough_cpu_counts_to_compare(per_cpu_count):
    assert len(per_cpu_count) >= 2, "needs a process that may use two CPUs at least"


@pytest.mark.parametrize("name", SCENES)
def test_tree_does_not_depend_on_the_cpu_count(per_cpu_count, name):
    ks = sorted(per_cpu_count)
    assert len(ks) >= 2
    base = per_cpu_count[ks[0]][name]
    print("%s: nodes, triangles, depth %s on %s CPUs" % (name, base["size"], ks))
    n = int(name.split("-")[1])
    assert abs(base["size"][1] - n) < 0.02 * n
    for k in ks[1:]:
        assert per_cpu_count[k][name]["size"] == base["size"], (k, ks[0])
        assert per_cpu_count[k][name]["leaf_sets"] == base["leaf_sets"], "leaf SETS differ between %d and %d CPUs" % (k, ks[0])
    for k in ks[1:]:
        for key in BYTE_KEYS:
            assert per_cpu_count[k][name][key] == base[key], "%s differs between %d and %d CPUs (the leaves' sets agree)" % (key, k, ks[0])


def test_leaves_are_in_input_order(hpt, sio):
    """The canonical order: inside a leaf the ordinals ascend."""
    bvh = hpt.export_bvh_host(*sio.cornell_random_triangles(20000))
    sets = leaf_sets(bvh)
    assert np.array_equal(sets[-bvh["num_tris"]:], bvh["tris"][:, 3].astype(np.int64))


# ---- the paths only large scenes take ------------------------------------------------------------------------------------

SIZES = [8192, 8193, 65535, 65536, 131071, 131072]          # kParallelMin is exclusive, kParallelForMin and kBigNode inclusive
WIN_W, WIN_H, WINDOW = 64, 48, (24, 18, 40, 30)             # a 16 x 12 window in the middle of the image


@pytest.fixture(scope="module")
def big_random(sio):
    L, sp, tr = sio.cornell_random_triangles(max(SIZES))
    tr.setflags(write=False)
    return L, sp, tr


@pytest.mark.parametrize("count", SIZES)
def test_big_scene_paths_build_a_tree_that_returns_the_scan(hpt, sio, oracle_mod, big_random, count):
    L, sp, tr = big_random
    tr = tr[:count]
    assert len(tr) == count
    bvh = hpt.export_bvh_host(L, sp, tr)
    _check_tree(bvh, count)
    assert np.array_equal(leaf_sets(bvh)[-count:], bvh["tris"][:, 3].astype(np.int64))
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, WIN_W, WIN_H)
    kw = dict(seed=23, window=WINDOW)
    scan, s_scan = oracle_mod.pt_render(L, sp, tr, cam, WIN_W, WIN_H, 3, 2, **kw)
    walk, s_walk = oracle_mod.pt_render(L, sp, tr, cam, WIN_W, WIN_H, 3, 2, bvh=bvh, **kw)
    assert (WINDOW[2] - WINDOW[0], WINDOW[3] - WINDOW[1]) == (16, 12) and s_scan["samples"] == 16 * 12 * 2
    assert scan.any() and not scan[:WINDOW[1]].any() and not scan[:, :WINDOW[0]].any()
    assert np.array_equal(walk, scan)
    assert all(s_walk[k] == s_scan[k] for k in ("closest_rays", "shadow_rays"))
    boxes = s_walk["boxes_closest"] / 2 / s_walk["closest_rays"]
    print("%d triangles: nodes %d, depth %d, boxes per closest ray %.1f" % (count, bvh["num_nodes"], bvh["bvh_depth"], boxes))
