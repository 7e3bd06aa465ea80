"""The device held to what the REFERENCE'S OWN CODE computed (tests/golden/ref_*.npz: the reference's sources built for the
host, tests/golden/make_ref_golden.py).  Fixtures only, no tolerance: every comparison is of bits.  The CPU side of the same
pin, which holds the oracle to these files on every column, is tests/test_reference_pin_cpu.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from kat_records import same_bits
from path_tracing_amd.layouts import CAMERA, LIGHT, SPHERE, TRIANGLE

pytestmark = pytest.mark.gpu


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _rec(raw, dtype):
    return np.ascontiguousarray(raw).view(dtype).reshape(-1)


def _scene(g, key):
    return _rec(g[key + "/lights"], LIGHT), _rec(g[key + "/spheres"], SPHERE), _rec(g[key + "/tris"], TRIANGLE)


RAY_SCENES = [str(s) for s in _load("ref_rays.npz")["scenes"]]
PT_CASES = [str(s) for s in _load("ref_pt_kernel.npz")["cases"]]

# Columns of the 40-float table whose reference expression calls no transcendental function, from reading geometric.cuh:
# bsdf_evaluate and bsdf_pdf (frame, GGX D / Lambda / G, both Fresnels) use + - * /, sqrtf, fabs, fmaxf, fminf and isinf
# only, and so do the guards, the frame and the Fresnel / GGX columns themselves.  sinf and cosf are called in two places:
# SampleTrowbridgeReitzVisibleNormal and the cosine lobe of bsdf_sample -- so the visible normal (22-24), the sin / cos
# columns (20-21) and, on records that take a ROUGH branch, bsdf_sample's wi / f / pdf (4-10) are left to the CPU test
# (oracle with libm trig == reference) and to test_function_kats.py (device == oracle with the shared polynomial).
# is_delta and new_eta (11-12) are set before any trigonometry on every branch; on a DELTA branch 4-10 are trig-free too.
TRIG_FREE = [0, 1, 2, 3, 11, 12, 13, 14, 15, 16, 17, 18, 19, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39]
TRIG_FREE_ON_DELTA = [4, 5, 6, 7, 8, 9, 10]
TRIG = [20, 21, 22, 23, 24]
assert sorted(TRIG_FREE + TRIG_FREE_ON_DELTA + TRIG) == list(range(40))


def test_device_functions_equal_the_reference_where_it_calls_no_transcendental(hpt):
    g = _load("ref_functions.npz")
    rec, ref = g["records"], g["table"]
    got = hpt.probe_functions(rec)
    ok = same_bits(got, ref)
    bad = ~ok[:, TRIG_FREE]
    assert not bad.any(), "columns %s, records %s" % (sorted({TRIG_FREE[c] for c in np.nonzero(bad)[1]}), sorted(set(np.nonzero(bad)[0]))[:20])
    delta = ref[:, 11] == 1.0
    assert delta.sum() > 200
    bad = ~ok[np.ix_(delta, TRIG_FREE_ON_DELTA)]
    assert not bad.any(), "delta records: columns %s, records %s" % (sorted({TRIG_FREE_ON_DELTA[c] for c in np.nonzero(bad)[1]}),
                                                                     sorted(set(np.nonzero(delta)[0][np.nonzero(bad)[0]]))[:20])


@pytest.mark.parametrize("name", RAY_SCENES)
def test_device_walk_and_scan_equal_the_reference(hpt, name):
    """Scene.trace_closest against find_closest_hit's (t, scan ordinal) and Scene.trace_visibility against check_visibility
    with mtl_old.refract = eta, Ks = 1 (what the device defines), through the tree and with brute_force."""
    g = _load("ref_rays.npz")
    L, sp, tr = _scene(g, name)
    o, d, p1, p2 = (g[name + "/" + k] for k in ("o", "d", "p1", "p2"))
    want_vis = g[name + "/vis_eta"][:, 0].astype(np.int32)
    with hpt.Scene(L, sp, tr) as scene:
        for brute in (False, True):
            t, prim = scene.trace_closest(o, d, brute_force=brute)
            vis = scene.trace_visibility(p1, p2, brute_force=brute)
            how = "scan" if brute else "tree"
            bad = np.nonzero((t.view(np.uint32) != g[name + "/t"].view(np.uint32)) | (prim != g[name + "/ordinal"]))[0]
            assert not len(bad), "%s: %d rays differ, first %d: device (%r, %d) reference (%r, %d)" % (
                how, len(bad), bad[0], t[bad[0]], prim[bad[0]], g[name + "/t"][bad[0]], g[name + "/ordinal"][bad[0]])
            bad = np.nonzero(vis != want_vis)[0]
            assert not len(bad), "%s: %d segments differ, first %d" % (how, len(bad), bad[0] if len(bad) else -1)


# input.txt is rendered by tests/pt_cases.py already (depths 1 to 40, five shapes, three seeds): its two cases are left out here
RENDER_CASES = [c for c in PT_CASES if not c.startswith("input-")]


@pytest.mark.parametrize("case", RENDER_CASES)
def test_render_equals_the_replay_pinned_oracle(hpt, oracle_mod, case):
    """On the scenes where the oracle's replay equals the reference's kernel bit for bit (test_reference_pin_cpu.py),
    render_pt equals the same oracle in counter mode: one code path of the oracle, pinned from both sides."""
    g = _load("ref_pt_kernel.npz")
    L, sp, tr = _scene(g, case)
    W, H, depth, spp, seed = (int(v) for v in g[case + "/params"])
    cam = _rec(g[case + "/camera"], CAMERA)[0]
    want, st = oracle_mod.pt_render(L, sp, tr, cam, W, H, depth, spp, seed=seed)
    assert st["max_delta_run"] <= 32
    with hpt.Scene(L, sp, tr) as scene:
        img = scene.render_pt(cam, W, H, depth, spp, hpt.make_params(seed=seed))
    bad = (img.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not bad.any(), "%d of %d pixels differ, max abs %g" % (bad.sum(), W * H, np.abs(img - want).max())
    assert want.max() > 0
