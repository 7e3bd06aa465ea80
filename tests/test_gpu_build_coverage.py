"""The tree builder's case table (build_cases.py) on the MI355X: for records with NaN, infinite and overflowing
coordinates, for the finite outliers that make a ray visit every node, and for junk spheres, the device holds the tree
the host build exports, walks it to the oracle's bytes, and counts the work the oracle's host walk counts.

tests/test_build_cases_cpu.py is the host half: it establishes, without a device, that every tree of the table is well
formed, that its grid is finite (but for live-overflow, whose grid is infinite on purpose: the device then walks NaN
planes) and that the host walk through it is the scan."""
import numpy as np
import pytest

import build_cases as bc
from test_bvh_walk import COUNT_KEYS

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in bc.CASES]
TREE_KEYS = ("qnodes", "tris", "qorigin", "qscale")
SIZE_KEYS = ("num_nodes", "num_tris", "num_rounds", "bvh_depth")


@pytest.mark.parametrize("name", NAMES)
def test_case_on_the_device(hpt, oracle_mod, name):
    args, ref, ref_st = bc.reference(oracle_mod, name)
    L, sp, tr, cam, W, H, depth, spp, kw = args
    host_tree = bc.tree(hpt, name)
    # the host half, once more: what goes to the device is finite (but for the one case named), and its host walk is bounded
    # and is the scan
    assert (name in bc.NON_FINITE_GRID) != bool(np.isfinite(host_tree["qorigin"]).all() and np.isfinite(host_tree["qscale"]).all())
    walk, walk_st = bc.oracle_render(oracle_mod, args, bvh=host_tree)
    assert np.array_equal(walk, ref)
    assert walk_st["boxes_closest"] <= 2 * host_tree["num_nodes"] * walk_st["closest_rays"]
    with hpt.Scene(L, sp, tr) as scene:
        dev_tree = scene.export_bvh()
        counted = scene.render_pt(cam, W, H, depth, spp, hpt.make_params(flags=hpt.FLAG_COUNT_WORK, **kw))
        st = scene.stats()
        plain = scene.render_pt(cam, W, H, depth, spp, hpt.make_params(**kw))          # two pipelines, LDS tree top, split trace budget
    for k in TREE_KEYS:
        assert dev_tree[k].dtype == host_tree[k].dtype and dev_tree[k].tobytes() == host_tree[k].tobytes(), k
    for k in SIZE_KEYS:
        assert dev_tree[k] == host_tree[k], k
    # the oracle through the DEVICE's tree (the same bytes, so the same walk)
    for what, img in (("counted", counted), ("default flags", plain)):
        print("%s, %s: %d of %d pixels differ" % (name, what, int((img != ref).any(axis=-1).sum()), W * H))
    got = {k: int(st[k]) for k in COUNT_KEYS}
    want = {k: int(walk_st[k]) for k in COUNT_KEYS}
    print("%s: work counts device %s, host walk %s" % (name, got, want))
    assert np.array_equal(counted, ref)
    assert got == want
    assert want["closest_rays"] == ref_st["closest_rays"] and want["shadow_rays"] == ref_st["shadow_rays"]
    assert np.array_equal(plain, ref)
