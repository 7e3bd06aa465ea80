"""The builder's case table (build_cases.py) on the host alone: export_bvh_host returns a well-formed tree for records
with NaN, infinite and overflowing coordinates, the oracle's walk of that tree returns the scan's bytes (also with every
reciprocal moved 1 and 2 float neighbours), the walk stays within the project's traversal gate, and the builder -- in
a stand-alone program under the address and undefined-behaviour sanitizers -- does nothing undefined on the way."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import build_cases as bc
from test_bvh_walk import _check_tree

NAMES = [c.name for c in bc.CASES]
RAYS = ("closest_rays", "shadow_rays")
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "path_tracing_amd", "csrc")


def _per_ray(st):
    return st["boxes_closest"] / 2 / max(st["closest_rays"], 1), st["tris_closest"] / max(st["closest_rays"], 1)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_says(oracle_mod, name):
    case = bc.CASE_BY_NAME[name]
    args, img, st = bc.reference(oracle_mod, name)
    L, sp, tr = args[:3]
    assert (args[4], args[5], args[6], args[7]) == (40, 32, 4, 3) and len(tr) <= bc.MAX_TRIS
    assert img.shape == (32, 40, 3) and np.isfinite(img).all() and img.min() >= 0.0
    lit = bc.lit_share(img)
    print("%s: N %d, lit %.3f, closest rays %d, shadow rays %d" % (name, len(tr), lit, st["closest_rays"], st["shadow_rays"]))
    assert img.any() and st["closest_rays"] >= st["samples"] == 40 * 32 * 3       # every case renders something
    if case.dark is None:
        assert lit >= 0.5 and st["shadow_rays"] > 0
    n_dead = {"plain": 0, "nan-one": 1, "nan-20-middle": 20, "nan-20-front": 20, "inf-one": 1, "inf-30": 30,
              "overflow-span": 3, "reach-1e30": 0, "reach-1e6": 0, "live-overflow": 0, "all-nan": 12, "junk-spheres": 0}[name]
    d = bc.dead(tr)
    assert d.sum() == n_dead
    if name == "nan-20-front":
        assert d[:20].all()
    if name == "nan-20-middle":
        assert d[len(tr) // 2 - 10:len(tr) // 2 + 10].all()
    if name == "overflow-span":
        assert all(np.isfinite(tr[k]).all() for k in ("v0", "v1", "v2"))
    if name in bc.FINITE_OUTLIERS:
        assert max(float(np.abs(tr[k]).max()) for k in ("v0", "v1", "v2")) in (1e6, float(np.float32(1e30)), float(np.float32(3e38)))
    if name == "junk-spheres":
        assert len(sp) == 4 and np.isnan(sp["center"]).sum() == 1 and np.isinf(sp["r"]).sum() == 1


def test_dark_cases_are_the_named_ones():
    assert {c.name for c in bc.CASES if c.dark} == set(bc.DARK)
    assert all(isinstance(c.dark, str) and len(c.dark) > 10 for c in bc.CASES if c.dark)
    assert len(bc.CASES) == 12 and set(bc.FINITE_OUTLIERS) < set(NAMES)


def test_dead_triangles_change_nothing_the_scan_returns(oracle_mod):
    """The premise of the builder's rule: the scan never hits a triangle with a non-finite edge, so the image and the ray
    counts are the base scene's whatever junk is added."""
    _, plain, s_plain = bc.reference(oracle_mod, "plain")
    for name in ("nan-one", "nan-20-middle", "nan-20-front", "inf-one", "inf-30", "overflow-span"):
        _, img, st = bc.reference(oracle_mod, name)
        assert np.array_equal(img, plain), name
        assert all(st[k] == s_plain[k] for k in RAYS), name


def test_denormal_scene_renders_nothing_and_is_not_a_case(oracle_mod):
    img, st = bc.oracle_render(oracle_mod, bc.denormal_case())
    assert not img.any() and st["shadow_rays"] == 0
    assert "denormal" not in " ".join(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_exported_tree_is_well_formed(hpt, name):
    tr = bc.CASE_BY_NAME[name].make()[2]
    bvh = bc.tree(hpt, name)
    _check_tree(bvh, len(tr))
    if name in bc.NON_FINITE_GRID:
        assert np.isneginf(bvh["qorigin"]).all() and np.isposinf(bvh["qscale"]).all()
    else:
        assert np.isfinite(bvh["qorigin"]).all() and np.isfinite(bvh["qscale"]).all() and (bvh["qscale"] > 0).all()
    assert 1 <= bvh["bvh_depth"] <= 30
    # the leaf-order records carry the input's v0 / e1 / e2 bit for bit, dead ones included
    ords = bvh["tris"][:, 3].astype(np.int64) - bvh["num_rounds"]
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.concatenate([tr["v0"], tr["v1"] - tr["v0"], tr["v2"] - tr["v0"]], axis=1).astype(np.float32)[ords]
    got = bvh["tris"][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    live = ~bc.dead(tr)[ords]
    assert np.array_equal(got[live], want.view(np.uint32)[live])
    assert np.array_equal(np.isfinite(got.view(np.float32)), np.isfinite(want))
    if name in bc.SAME_TREE_AS_PLAIN:
        plain = bc.tree(hpt, "plain")
        assert all(np.array_equal(bvh[k], plain[k]) for k in ("qnodes", "qorigin", "qscale"))
        assert np.array_equal(np.delete(bvh["tris"], [3, 7], axis=1), np.delete(plain["tris"], [3, 7], axis=1))      # (ordinals and material numbers move: the spheres come first)


def test_grid_ignores_dead_triangles(hpt):
    """A record no ray can hit moves neither the grid nor the scene's box: the grid is the base scene's, and so is the
    union of the root's two child boxes (all 16 bits of the grid on every axis)."""
    plain = bc.tree(hpt, "plain")

    def root_box(bvh):
        w = bvh["qnodes"][0, :6]
        return np.minimum(w & 0xFFFF, w >> 16)[0::2], np.maximum(w & 0xFFFF, w >> 16)[1::2]

    assert np.array_equal(root_box(plain)[0], [0, 0, 0]) and np.array_equal(root_box(plain)[1], [65535] * 3)
    for name in ("nan-one", "nan-20-middle", "nan-20-front", "inf-one", "inf-30", "overflow-span"):
        bvh = bc.tree(hpt, name)
        assert np.array_equal(bvh["qorigin"], plain["qorigin"]) and np.array_equal(bvh["qscale"], plain["qscale"]), name
        assert all(np.array_equal(a, b) for a, b in zip(root_box(bvh), root_box(plain))), name


@pytest.mark.parametrize("name", NAMES)
def test_walk_of_the_exported_tree_equals_the_scan(hpt, oracle_mod, name):
    """Bytes and ray counts; then again with the three reciprocals of every ray moved 1 and 2 ulps in each of the 8
    combinations of directions; then the traversal gate of SURVEY 8(d) (test_bvh_walk.py): mean boxes per closest-hit
    ray <= 3 log2(N), N the triangle count -- for every case but the finite outliers (bc.FINITE_OUTLIERS: the two reaches
    and live-overflow), whose counts are printed."""
    args, scan, s_scan = bc.reference(oracle_mod, name)
    bvh = bc.tree(hpt, name)
    walk, s_walk = bc.oracle_render(oracle_mod, args, bvh=bvh)
    boxes, tris = _per_ray(s_walk)
    print("%s: nodes %d, depth %d, boxes per closest ray %.1f, triangles per closest ray %.1f"
          % (name, bvh["num_nodes"], bvh["bvh_depth"], boxes, tris))
    assert np.array_equal(walk, scan)
    assert all(s_walk[k] == s_scan[k] for k in RAYS)
    assert s_walk["boxes_closest"] >= 2 * s_walk["closest_rays"]
    for ulps in (1, 2):
        for mask in range(8):
            img, st = bc.oracle_render(oracle_mod, args, bvh=bvh, rcp_nudge=(ulps, mask))
            assert np.array_equal(img, scan), (ulps, mask)
            assert all(st[k] == s_scan[k] for k in RAYS), (ulps, mask)
    if name not in bc.FINITE_OUTLIERS:
        assert boxes <= 3.0 * np.log2(len(args[2])), boxes


# ---- undefined behaviour: the builder alone, under the sanitizers ------------------------------------------------------

SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def build_check(tmp_path_factory):
    """tests/build_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in.  Their runtimes
    are linked statically (clang's default; asked of g++), so the program stands on its own in whatever environment
    the suite runs in."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("build_check") / "build_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "build_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    return exe


def _write_records(path, L, sp, tr):
    L, sp, tr = np.ascontiguousarray(L), np.ascontiguousarray(sp), np.ascontiguousarray(tr)
    assert (L.dtype.itemsize, sp.dtype.itemsize, tr.dtype.itemsize) == (144, 100, 120)
    with open(path, "wb") as f:
        f.write(np.array([len(L), len(sp), len(tr)], np.int32).tobytes())
        f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())


@pytest.mark.parametrize("name", NAMES)
def test_builder_is_clean_under_the_sanitizers(hpt, build_check, tmp_path, name):
    L, sp, tr = bc.CASE_BY_NAME[name].make()[:3]
    rec = str(tmp_path / "records.bin")
    _write_records(rec, L, sp, tr)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([build_check, rec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    # the program prints what it built: the same tree as the library's
    out = dict(kv.split("=") for kv in p.stdout.decode().split())
    bvh = bc.tree(hpt, name)
    assert (int(out["nodes"]), int(out["tris"]), int(out["depth"])) == (bvh["num_nodes"], bvh["num_tris"], bvh["bvh_depth"])
    assert int(out["qnodes_fnv"], 16) == _fnv(bvh["qnodes"].tobytes()) and int(out["tris_fnv"], 16) == _fnv(bvh["tris"].tobytes())


def _fnv(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h
