"""k_trace's deep stacks on the device: the cases of walk_cases.py, on which the host restatement of the kernel
(tests/walk_check.cpp, held in test_walk_cases_cpu.py) proves that every primary ray holds 36 or more entries of the four-wide
stack -- stores to and loads from the global-memory column, steps that write LDS and global levels at once -- that the tree
of onion-unsplit is too deep to be split, and that onion-binary fills the binary walk's LDS stack to 26 of kStackDepth.

Every image is oracle.pt_render's bit for bit (the scan: no tree), every count the oracle's host walk of the exported tree;
which trees are split comes from walk_cases.CASES, which test_walk_cases_cpu.py holds to the walker."""
import numpy as np
import pytest

import walk_cases as wc
from test_bvh_walk import COUNT_KEYS
from test_gpu_bdpt_coverage import bdpt_parity
from test_gpu_ppm_coverage import olib, ppm_parity              # noqa: F401  (olib is a fixture)

pytestmark = pytest.mark.gpu

W, H, DEPTH, SPP, SEED = wc.W, wc.H, wc.DEPTH, wc.SPP, wc.SEED
NO_SPLIT = 63                                                  # hpt_params.reserved bits 1-6: 0 = default, 63 = one launch
BUDGETS = (1, 0, 7, 12, 32, NO_SPLIT)
_REF = {}


def reference(oracle_mod, name, step=-1, roulette=False):
    """(records, camera, image) of a case's state by the oracle's scan, once per process; callers must not write to them."""
    key = (name, step, roulette)
    if key not in _REF:
        c = wc.CASE_BY_NAME[name]
        L, sp, tr = c.make()
        if step >= 0:
            tr = c.steps()[step]
        img, _ = oracle_mod.pt_render(L, sp, tr, c.camera(), W, H, DEPTH, SPP, seed=SEED, russian_roulette=roulette)
        img.setflags(write=False)
        _REF[key] = ((L, sp, tr), c.camera(), img)
    return _REF[key]


def render(hpt, scene, cam, flags=0, budget=0):
    p = hpt.make_params(seed=SEED, flags=flags)
    p.reserved = budget << 1
    return scene.render_pt(cam, W, H, DEPTH, SPP, p)


def expected_split(fits, budget):
    return 0 if (not fits or budget == NO_SPLIT) else (wc.TRACE_BUDGET if budget == 0 else budget)


def same(img, ref, what):
    assert img.shape == ref.shape
    assert np.array_equal(img, ref), "%s: %d pixels differ, max abs %.3e" % (what, int((img != ref).any(axis=-1).sum()), float(np.abs(img - ref).max()))


@pytest.mark.parametrize("name", wc.NAMES)
def test_every_budget_gives_the_oracles_image(hpt, oracle_mod, name):
    """With TIME_KERNELS the stats tell what was launched: the requested budget and a resume launch where the walker says the
    tree fits, one launch per step where it does not, whatever is requested."""
    (L, sp, tr), cam, ref = reference(oracle_mod, name)
    fits = wc.CASE_BY_NAME[name].fits
    with hpt.Scene(L, sp, tr) as scene:
        for budget in BUDGETS:
            img = render(hpt, scene, cam, hpt.FLAG_TIME_KERNELS, budget)
            st = scene.stats()
            same(img, ref, "%s, budget %d" % (name, budget))
            assert st["split_budget"] == expected_split(fits, budget), (name, budget, st["split_budget"])
            assert (st["n_resume"] > 0) == (expected_split(fits, budget) != 0), (name, budget, st["n_resume"])


@pytest.mark.parametrize("name", wc.NAMES)
def test_flag_sets_give_the_oracles_image(hpt, oracle_mod, name):
    """NO_HOST_WAIT: the blind tail's capped grid makes the resume launch stride over chunks on one column of the deep stack."""
    (L, sp, tr), cam, ref = reference(oracle_mod, name)
    with hpt.Scene(L, sp, tr) as scene:
        for flags in (0, hpt.FLAG_SINGLE_PIPELINE, hpt.FLAG_NO_HOST_WAIT, hpt.FLAG_SINGLE_PIPELINE | hpt.FLAG_NO_HOST_WAIT, hpt.FLAG_BRUTE_FORCE):
            same(render(hpt, scene, cam, flags), ref, "%s, flags %d" % (name, flags))
        same(render(hpt, scene, cam, hpt.FLAG_RUSSIAN_ROULETTE), reference(oracle_mod, name, roulette=True)[2], "%s, roulette" % name)
        same(render(hpt, scene, cam, 0, 1), ref, "%s, after the other flags" % name)


@pytest.mark.parametrize("name", wc.NAMES)
def test_work_counts_equal_the_host_walk(hpt, oracle_mod, name):
    (L, sp, tr), cam, ref = reference(oracle_mod, name)
    with hpt.Scene(L, sp, tr) as scene:
        tree = scene.export_bvh()
        img = render(hpt, scene, cam, hpt.FLAG_COUNT_WORK)
        st = scene.stats()
    host = hpt.export_bvh_host(L, sp, tr)
    for k in ("qnodes", "tris", "qorigin", "qscale"):
        assert np.array_equal(tree[k], host[k]), k
    walk, so = oracle_mod.pt_render(L, sp, tr, cam, W, H, DEPTH, SPP, seed=SEED, bvh=tree)
    same(walk, ref, name + ", the oracle through the tree")
    same(img, ref, name + ", counting")
    assert {k: int(st[k]) for k in COUNT_KEYS} == {k: int(so[k]) for k in COUNT_KEYS}
    assert st["split_budget"] == 0


def test_ppm_on_the_deep_onion(hpt, oracle_mod, olib):                    # noqa: F811
    """render_ppm.cpp's eye pass uses the same two launches."""
    (L, sp, tr), cam, _ = reference(oracle_mod, "onion-deep")
    ppm_parity(hpt, olib, L, sp, tr, cam, W, H, eye_depth=3, light_depth=3, spp=1, spl=32, radius=0.05, seed=SEED)


def test_ppm_where_bounce_rays_go_deep(hpt, oracle_mod, olib):            # noqa: F811
    """coarse: the rays from the first hits on hold 30 entries and more (the walker's R and S families), so the resume launch
    walks deep from records and from shadow-queue entries, not from primary rays alone."""
    (L, sp, tr), cam, _ = reference(oracle_mod, "coarse")
    ppm_parity(hpt, olib, L, sp, tr, cam, W, H, eye_depth=4, light_depth=3, spp=1, spl=32, radius=0.05, seed=SEED)


def test_ppm_on_the_unsplit_onion(hpt, oracle_mod, olib):                 # noqa: F811
    """No resume launch here: the one-launch fallback of render_ppm.cpp."""
    (L, sp, tr), cam, _ = reference(oracle_mod, "onion-unsplit")
    ppm_parity(hpt, olib, L, sp, tr, cam, W, H, eye_depth=3, light_depth=3, spp=1, spl=32, radius=0.05, seed=SEED)


def test_bdpt_on_the_deepest_binary_tree(hpt, sio, oracle_mod):
    """The bidirectional walk keeps bvh_depth + 1 levels in LDS (kStackDepth at most); one group holds everything, so its tree
    is the builder's tree of the same triangles."""
    L, sp, tr = wc.CASE_BY_NAME["onion-binary"].make()
    assert hpt.export_bvh_host(L, sp, tr)["bvh_depth"] == wc.MAX_BVH_DEPTH
    order = sio.object_order(None, sp, tr)
    view = ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), sio.CORNELL_UP, wc.ONION_FOV)
    args = (L, sp, tr, order, view, W, H, 3, 2, 2, 4, SEED, 0)
    ref, rst = oracle_mod.bdpt_render(L, sp, tr, order, view[0], view[1], view[2], view[3], W, H, 3, 2, 2, 4, seed=SEED)
    assert wc.lit_share(ref) >= 0.10
    bdpt_parity(hpt, sio, args, ref, rst)


@pytest.mark.parametrize("name", ["onion-cap", "coarse", "onion-far"])
def test_refit_then_rebuild_of_a_deep_split_tree(hpt, oracle_mod, name):
    """The sizes reversed: the refit keeps the topology, whose boxes then nest the other way round; the rebuild gives the
    builder's tree of the new records.  test_walk_cases_cpu.py holds what the walker finds on the refitted trees: primary rays
    of onion-cap hold 36 entries or more; on coarse, bounce and shadow rays reach the global levels and the blocker of a
    quarter and more of the shadow rays lies under a node popped from deep[]; on onion-far a quarter and more of the primary
    rays (the walker: 79 %) pop a far subtree from a global level, miss all four children, take the `top` that level() loaded
    from a global level and find their final hit under it -- a wrong word from that load is another image."""
    c = wc.CASE_BY_NAME[name]
    (L, sp, tr), cam, ref = reference(oracle_mod, name)
    moved, _, ref_moved = reference(oracle_mod, name, 0)
    with hpt.Scene(L, sp, tr) as scene:
        same(render(hpt, scene, cam, hpt.FLAG_TIME_KERNELS), ref, "built")
        assert scene.stats()["split_budget"] == wc.TRACE_BUDGET
        scene.update_triangles(moved[2])
        for budget in (0, 1):
            same(render(hpt, scene, cam, hpt.FLAG_TIME_KERNELS, budget), ref_moved, "refitted, budget %d" % budget)
            st = scene.stats()
            assert st["split_budget"] == expected_split(c.fits, budget) and st["n_resume"] > 0          # the topology, so the verdict, is kept
        scene.rebuild()
        assert np.array_equal(scene.export_bvh()["qnodes"], hpt.export_bvh_host(*moved)["qnodes"])
        for budget in (0, 1):
            same(render(hpt, scene, cam, hpt.FLAG_TIME_KERNELS, budget), ref_moved, "rebuilt, budget %d" % budget)
            assert scene.stats()["split_budget"] == expected_split(c.fits_rebuilt[0], budget)


def test_the_split_comes_and_goes_with_the_tree(hpt, oracle_mod):
    """onion-unsplit: too deep; flattened and rebuilt: split; moved back and rebuilt: too deep again.  A refit alone keeps the
    tree, so the verdict."""
    name = "onion-unsplit"
    c = wc.CASE_BY_NAME[name]
    (L, sp, tr), cam, ref = reference(oracle_mod, name)
    flat, _, ref_flat = reference(oracle_mod, name, 0)
    assert (c.fits, c.fits_rebuilt[:2]) == (False, (True, False)) and np.array_equal(c.steps()[1], tr)

    def check(scene, want, split, what):
        same(render(hpt, scene, cam, hpt.FLAG_TIME_KERNELS), want, what)
        st = scene.stats()
        assert st["split_budget"] == (wc.TRACE_BUDGET if split else 0) and (st["n_resume"] > 0) == split, (what, st["split_budget"], st["n_resume"])
    with hpt.Scene(L, sp, tr) as scene:
        check(scene, ref, False, "built")
        scene.update_triangles(flat[2])
        check(scene, ref_flat, False, "flattened, the deep tree refitted")
        scene.rebuild()
        check(scene, ref_flat, True, "flattened and rebuilt")
        scene.update_triangles(tr)
        check(scene, ref, True, "moved back, the shallow tree refitted")
        scene.rebuild()
        check(scene, ref, False, "moved back and rebuilt")


@pytest.mark.parametrize("name", ["onion-cap", "onion-unsplit"])
def test_a_posed_deep_tree_is_walked(hpt, oracle_mod, name):
    """One part, a scale of 1/2 about the origin (the eye): the device refits both trees (refit_kernels.hip) and every nested
    box still contains the eye, so the walks are as deep as before -- the resume walk on onion-cap, the one launch on
    onion-unsplit.  The records are pose_host's; the image is the oracle's for them."""
    c = wc.CASE_BY_NAME[name]
    step = wc.HALF_STEP[name]
    (L, sp, tr), cam, _ = reference(oracle_mod, name)
    (_, _, scaled), _, want = reference(oracle_mod, name, step)
    half = np.array([[0.5, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, 0.5, 0]], np.float32)[None]
    posed = hpt.pose_host(tr, None, half)
    assert posed.tobytes() == np.ascontiguousarray(scaled).tobytes()          # the records the walker walked as a refit step
    with hpt.Scene(L, sp, tr) as scene:
        scene.set_parts(None, 1)
        scene.pose(half)
        for budget in (0, 1):
            same(render(hpt, scene, cam, hpt.FLAG_TIME_KERNELS, budget), want, "%s posed, budget %d" % (name, budget))
            assert scene.stats()["split_budget"] == expected_split(c.fits, budget)
        scene.rebuild()
        for budget in (0, 1):
            same(render(hpt, scene, cam, hpt.FLAG_TIME_KERNELS, budget), want, "%s posed and rebuilt, budget %d" % (name, budget))
            assert scene.stats()["split_budget"] == expected_split(c.fits_rebuilt[step], budget)
