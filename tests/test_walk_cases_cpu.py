"""k_trace restated ray by ray on the host (tests/walk_check.cpp, built with csrc/scene_build.cpp under the address and
undefined-behaviour sanitizers, run as a program) on the cases of walk_cases.py:

  (a) on every case, refit step, ray family (P primary, R bounce, S shadow), budget in {0, 1, kTraceBudget, 7, 12, 32} and
      reciprocal (exact, and moved one float neighbour in each of the eight sign combinations) the walker's closest hit is
      oracle.closest_hits' -- t bit for bit, same ordinal -- and its any-hit result is oracle.visibility's: the binary and the
      four-wide tree, refitted ones included, are conservative ray by ray, and the restatement's arithmetic is the oracle's;
  (b) the cases reach what they are there for -- stack depths derived from kResumeLdsLevels, kDeepLevels and kMaxBvhDepth --
      under every one of the nine reciprocals;
  (c) the same walk on the scenes of test_resume_launch_walks_deep_trees_bit_exact and of deep_far_case: hits equal the
      oracle's, the stack depths are printed ("The walker");
  (d) in each deep case at least a quarter of the primary rays that reach level 12 hold other words in the global levels than
      the ray one pixel to the right;
  (e) at least 10 % of the pixels of every rendered state's oracle image are lit.

A reach condition is evaluated at budgets 1 and kTraceBudget: with a budget of 1 every ray that takes more than one node step
is set aside, so the four-wide walk starts with nothing found; every P ray of the onion cases is set aside at both."""
import os
import re

import numpy as np
import pytest

import pt_cases
import walk_cases as wc

_WALKED = {}


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_check")
    return wc.build_walker(d), d


def walked(oracle_mod, walker, name):
    """One run of the program per case and process: every step's rays, the trees' figures, the results per reciprocal and
    step, and the oracle's answers per step."""
    if name not in _WALKED:
        c = wc.CASE_BY_NAME[name]
        L, sp, tr = c.make()
        steps = c.steps()
        rays = [wc.ray_families(oracle_mod, L, sp, t, c.camera()) for t in [tr] + steps]
        trees, res = wc.run_walker(walker[0], walker[1], L, sp, tr, steps, rays)
        want = [answers(oracle_mod, L, sp, t, r) for t, r in zip([tr] + steps, rays)]
        _WALKED[name] = (rays, trees, res, want)
    return _WALKED[name]


def answers(oracle_mod, L, sp, tr, rays):
    c, a = rays.any == 0, rays.any == 1
    t, prim = oracle_mod.closest_hits(L, sp, tr, rays.ro[c], rays.rd[c])
    vis = oracle_mod.visibility(sp, tr, rays.ro[a], rays.p2[a])
    return t, prim, vis


def same_as_the_oracle(what, rays, res, want, bvh_depth, fits):
    """res: [rays, budgets]"""
    t, prim, vis = want
    c, a = rays.any == 0, rays.any == 1
    for bi, budget in enumerate(wc.BUDGETS):
        q = res[:, bi]
        assert not (q["flags"] & ((wc.WIDE_OVERRUN if fits else 0) | wc.BINARY_OVERRUN)).any(), (what, budget)
        bad = (q["t"][c] != t.view(np.uint32)) | (q["ord"][c].view(np.int32) != prim)
        assert not bad.any(), "%s, budget %d: %d closest hits differ, first ray %d: walker (%r, %d), oracle (%r, %d)" % (
            what, budget, bad.sum(), np.flatnonzero(bad)[0], q["t"][c][bad][:1].view(np.float32)[0], q["ord"][c].view(np.int32)[bad][0], t[bad][0], prim[bad][0])
        bad = (q["t"][a] != 0) != (vis == 0)
        assert not bad.any(), "%s, budget %d: %d any-hit results differ, first ray %d" % (what, budget, bad.sum(), np.flatnonzero(bad)[0])
        # what the launchers size: bvh_depth + 1 LDS levels in the first launch, budget + 1 when that is less (the store at
        # stk[sp] touches level sp); kResumeLdsLevels + kDeepLevels in the resume walk of a tree that fits
        assert q["max_sp1"].max() <= max(bvh_depth, 1) and (budget == 0 or q["max_sp1"].max() <= budget), (what, budget)
        if budget == 0:
            assert not (q["flags"] & wc.SET_ASIDE).any() and not q["steps2"].any()
        elif fits:
            assert q["max_sp2"].max() <= wc.RESUME_LDS_LEVELS + wc.DEEP_LEVELS, (what, budget)


def test_constants_are_the_headers():
    with open(os.path.join(wc.CSRC, "pt_kernels.h")) as f:
        kernels = f.read()
    with open(os.path.join(wc.CSRC, "hpt_scene.h")) as f:
        scene = f.read()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "walk_check.cpp")) as f:
        prog = f.read()

    def const(text, name):
        m = re.search(r"constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*(\w+)\s*;" % name, text)
        assert m, name
        return m.group(1)
    assert int(const(kernels, "kResumeLdsLevels")) == wc.RESUME_LDS_LEVELS == int(const(prog, "kResumeLdsLevels"))
    assert int(const(kernels, "kDeepLevels")) == wc.DEEP_LEVELS == int(const(prog, "kDeepLevels"))
    assert const(kernels, "kTraceBudget") == "HPT_TRACE_BUDGET" and int(re.search(r"#define HPT_TRACE_BUDGET (\d+)", kernels).group(1)) == wc.TRACE_BUDGET
    assert const(kernels, "kTopLevels") == "HPT_TOP_LEVELS" and int(re.search(r"#define HPT_TOP_LEVELS (\d+)", kernels).group(1)) == wc.TOP_LEVELS
    assert int(const(scene, "kMaxBvhDepth")) == wc.MAX_BVH_DEPTH and int(const(scene, "kStackDepth")) == wc.STACK_DEPTH
    assert "3 * sc.wide_depth + 2 <= kResumeLdsLevels + kDeepLevels" in kernels
    assert wc.RESULT.itemsize == 4 * int(const(prog, "kWords"))
    assert wc.TRACE_BUDGET in wc.BUDGETS and set(wc.BUDGETS) == {0, 1, wc.TRACE_BUDGET, 7, 12, 32}


@pytest.mark.parametrize("name", wc.NAMES)
def test_a_walker_equals_the_oracle(oracle_mod, walker, name):
    rays, trees, res, want = walked(oracle_mod, walker, name)
    c = wc.CASE_BY_NAME[name]
    assert [bool(t["fits"]) for t in trees] == [c.fits] * len(trees)          # a refit keeps the topology, so the verdict
    assert all(wc.fits(t) == bool(t["fits"]) for t in trees)
    assert all(len(r.ro) >= 5 * wc.W * wc.H + wc.N_BOUNCE for r in rays)
    for k, nudge in enumerate(wc.NUDGES):
        for s in range(len(rays)):
            same_as_the_oracle("%s, step %d, nudge %d" % (name, s - 1, nudge), rays[s], res[k][s], want[s], trees[s]["bvh_depth"], c.fits)


@pytest.mark.parametrize("name", [c.name for c in wc.CASES if c.fits_rebuilt])
def test_the_table_of_rebuilt_states_is_the_walkers(oracle_mod, walker, name):
    """walk_cases.CASES says whether the builder's tree of every step's records fits (test_gpu_deep_stack.py rebuilds there)."""
    c = wc.CASE_BY_NAME[name]
    L, sp, _ = c.make()
    rays = walked(oracle_mod, walker, name)[0]
    for s, tr in enumerate(c.steps()):
        few = wc.Rays(*[getattr(rays[s + 1], k)[:64] for k in wc.Rays._fields])
        trees, _ = wc.run_walker(walker[0], walker[1], L, sp, tr, [], [few], budgets=(0,), nudges=(-1,))
        print("%s, step %d built afresh: %r" % (name, s, trees[0]))
        assert bool(trees[0]["fits"]) == c.fits_rebuilt[s]


def _family(rays, res, fam, bi):
    return res[rays.family == fam, bi]


@pytest.mark.parametrize("name", wc.NAMES)
def test_b_cases_reach_what_they_are_for(oracle_mod, walker, name):
    rays, trees, res, _ = walked(oracle_mod, walker, name)
    c = wc.CASE_BY_NAME[name]
    tree = trees[0]
    split = [wc.BUDGETS.index(1), wc.BUDGETS.index(wc.TRACE_BUDGET)]
    half = wc.RESUME_LDS_LEVELS + wc.DEEP_LEVELS // 2
    assert half == 36
    for k, nudge in enumerate(wc.NUDGES):
        r = res[k][0]
        if nudge == -1:
            for fam in "PRS":
                b0, b1, bd = _family(rays[0], r, fam, 0), _family(rays[0], r, fam, split[0]), _family(rays[0], r, fam, split[1])
                paths = int(np.bitwise_or.reduce(b1["paths"])) | int(np.bitwise_or.reduce(bd["paths"]))
                print("%s %s: binary stack (unsplit) %d..%d; four-wide stack %d..%d at budget 1, %d..%d at budget %d; reached: %s" % (
                    name, fam, b0["max_sp1"].min(), b0["max_sp1"].max(), b1["max_sp2"].min(), b1["max_sp2"].max(), bd["max_sp2"].min(), bd["max_sp2"].max(),
                    wc.TRACE_BUDGET, ", ".join(n for n, bit in wc.PATHS.items() if paths & bit)))
        for bi in split:
            p = _family(rays[0], r, "P", bi)
            if c.deep or name == "onion-unsplit":
                # (the walker walks the four-wide tree of onion-unsplit too: the library does not, test_gpu_deep_stack.py)
                assert (p["flags"] & wc.SET_ASIDE).all()
            if c.deep:
                assert p["max_sp2"].min() >= half, (name, nudge, wc.BUDGETS[bi], p["max_sp2"].min())
                assert (p["deep_stores"] >= 1).all() and (p["deep_loads"] >= 1).all()
                # a step that stacks up to three cannot take sp from below 9 to 12: the step meant is one that writes LDS
                # levels and global levels at once, which level() serves with both of its branches
                assert (p["paths"] & wc.PATHS["level(): LDS and global in one step"]).any()
                assert (p["paths"] & wc.PATHS["leaf pop from deep[]"]).any()
            if name == "onion-cap":
                # the refitted trees the GPU tests render: reversed sizes (step 0) and the pose by one half (step 1)
                for s in (1, 2):
                    q = _family(rays[s], res[k][s], "P", bi)
                    assert (q["flags"] & wc.SET_ASIDE).all() and q["max_sp2"].min() >= half, (name, s - 1, nudge, q["max_sp2"].min())
                    if nudge == -1 and bi == split[0]:
                        print("%s step %d P: four-wide stack %d..%d" % (name, s - 1, q["max_sp2"].min(), q["max_sp2"].max()))
            if name == "onion-unsplit":
                q = _family(rays[3], res[k][3], "P", 0)                       # posed by one half: the one launch's walk is as deep
                assert q["max_sp1"].min() >= _family(rays[0], r, "P", 0)["max_sp1"].min() >= wc.RESUME_LDS_LEVELS
            if name == "coarse":
                # the conditions the issue sets for the sheets
                want = wc.RESUME_LDS_LEVELS + 3
                for s in (0, 1):
                    fam = {f: _family(rays[s], res[k][s], f, bi) for f in "PRS"}
                    assert (fam["P"]["flags"] & wc.SET_ASIDE).all() and fam["P"]["max_sp2"].min() >= want
                    shares = {f: float((fam[f]["max_sp2"] >= want).mean()) for f in "RS"}
                    if nudge == -1:
                        print("coarse step %d, budget %d: P %d..%d; R %d..%d, %.0f %% reach %d; S %d..%d, %.0f %% reach %d" % (
                            s - 1, wc.BUDGETS[bi], fam["P"]["max_sp2"].min(), fam["P"]["max_sp2"].max(), fam["R"]["max_sp2"].min(), fam["R"]["max_sp2"].max(),
                            100 * shares["R"], want, fam["S"]["max_sp2"].min(), fam["S"]["max_sp2"].max(), 100 * shares["S"], want))
                    assert shares["R"] >= 0.5 and shares["S"] >= 0.5, (name, s - 1, nudge, shares)
                    for f in "RS":
                        assert (fam[f]["deep_stores"] >= 1).mean() >= 0.5 and (fam[f]["paths"] & wc.PATHS["leaf pop from deep[]"]).any()
                # ... and on the refitted tree the any-hit walk's loads from global levels decide occlusion: the blocker of at
                # least a quarter of the S rays (the share condition (d) asks of differing neighbours: enough to show in an
                # image) lies under a node popped from deep[]
                s_ray = _family(rays[1], res[k][1], "S", bi)
                late = ((s_ray["paths"] & wc.PATHS["result found under a leaf pop from deep[]"]) != 0) & (s_ray["t"] != 0)
                if nudge == -1:
                    print("coarse step 0, budget %d: %d of %d S rays are blocked, %d of them by a triangle under a leaf pop from deep[]"
                          % (wc.BUDGETS[bi], (s_ray["t"] != 0).sum(), len(s_ray), late.sum()))
                assert late.mean() >= 0.25, (nudge, late.mean())
            if name == "onion-far":
                # refitted to the reversed sizes: the value level() loads from a global level as `top` is taken as the next node,
                # and the ray's final hit lies under it: at least a quarter of the primary rays (as above)
                q = _family(rays[1], res[k][1], "P", bi)
                took = (q["paths"] & wc.PATHS["miss pop from global"]) != 0
                decides = (q["paths"] & wc.PATHS["result found under a miss pop from global"]) != 0
                if nudge == -1:
                    print("onion-far step 0, budget %d: P four-wide stack %d..%d, %d of %d rays take the miss pop from a global level, %d find their final hit under it"
                          % (wc.BUDGETS[bi], q["max_sp2"].min(), q["max_sp2"].max(), took.sum(), len(q), decides.sum()))
                assert (q["paths"][took] & wc.PATHS["top read from global"]).all() and not (decides & ~took).any()
                assert decides.mean() >= 0.25 and (q["prim"][decides] != 0xFFFFFFFF).all(), (nudge, decides.mean())
        if name == "onion-cap":
            assert tree["wide_depth"] == 19 and tree["fits"] == 1 and 3 * 20 + 2 > wc.RESUME_LDS_LEVELS + wc.DEEP_LEVELS
        if name == "onion-unsplit":
            assert tree["wide_depth"] >= 20 and tree["fits"] == 0
        if name == "onion-binary":
            assert tree["bvh_depth"] == wc.MAX_BVH_DEPTH
            assert _family(rays[0], r, "P", 0)["max_sp1"].min() >= wc.MAX_BVH_DEPTH - 4


@pytest.mark.parametrize("name", wc.DIFFERENT_NEIGHBOURS)
def test_d_neighbouring_rays_hold_different_stacks(oracle_mod, walker, name):
    rays, _, res, _ = walked(oracle_mod, walker, name)
    for bi in (wc.BUDGETS.index(1), wc.BUDGETS.index(wc.TRACE_BUDGET)):
        p = _family(rays[0], res[0][0], "P", bi).reshape(len(wc.P_JITTERS), wc.H, wc.W)
        h = p["hash_lo"].astype(np.uint64) | (p["hash_hi"].astype(np.uint64) << np.uint64(32))
        reach = (p["max_sp2"] > wc.RESUME_LDS_LEVELS)[:, :, :-1]
        differ = (h[:, :, :-1] != h[:, :, 1:]) & reach
        share = differ.sum() / float(reach.sum())
        print("%s, budget %d: %d of the %d P rays with a right neighbour reach level %d, %.1f %% of those hold other words than it"
              % (name, wc.BUDGETS[bi], reach.sum(), reach.size, wc.RESUME_LDS_LEVELS, 100.0 * share))
        assert reach.sum() > 0 and share >= 0.25


@pytest.mark.parametrize("name", wc.NAMES)
def test_e_rendered_states_are_lit(oracle_mod, name):
    c = wc.CASE_BY_NAME[name]
    L, sp, tr = c.make()
    for s, t in enumerate([tr] + c.steps()):
        img, _ = oracle_mod.pt_render(L, sp, t, c.camera(), wc.W, wc.H, wc.DEPTH, wc.SPP, seed=wc.SEED)
        print("%s, step %d: %.1f %% of the pixels lit" % (name, s - 1, 100.0 * wc.lit_share(img)))
        assert wc.lit_share(img) >= 0.10


def _benchmark_shaped(sio):
    cam = sio.make_camera(sio.CORNELL_EYE, sio.CORNELL_LOOK, sio.CORNELL_UP, 50.0, 80, 64)
    L, sp, tr, fcam, fw, fh = pt_cases.deep_far_case()[:6]
    return [("cornell_with_sphere(30000)", sio.cornell_with_sphere(30000), cam, 80, 64),
            ("cornell_random_triangles(20000)", sio.cornell_random_triangles(20000), cam, 80, 64),
            ("deep-far", (L, sp, tr), fcam, fw, fh)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_c_benchmark_shaped_scenes_hold_shallow_stacks(oracle_mod, walker, sio, which):
    """Nothing is asserted about the depths: they are what DESIGN.md and the docstrings of the two tests quote."""
    what, (L, sp, tr), cam, w, h = _benchmark_shaped(sio)[which]
    rays = wc.ray_families(oracle_mod, L, sp, tr, cam, w, h)
    trees, res = wc.run_walker(walker[0], walker[1], L, sp, tr, [], [rays], nudges=(-1,))
    r = res[0][0]
    same_as_the_oracle(what, rays, r, answers(oracle_mod, L, sp, tr, rays), trees[0]["bvh_depth"], True)
    b1 = wc.BUDGETS.index(1)
    print("%s: bvh_depth %d, wide_depth %d; deepest stack of %d rays: binary (unsplit) %d, four-wide %d at budget 1, %d at budget %d"
          % (what, trees[0]["bvh_depth"], trees[0]["wide_depth"], len(rays.ro), r[:, 0]["max_sp1"].max(), r[:, b1]["max_sp2"].max(),
             r[:, wc.BUDGETS.index(wc.TRACE_BUDGET)]["max_sp2"].max(), wc.TRACE_BUDGET))
