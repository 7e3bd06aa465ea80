"""The case table of the bidirectional coverage suite (bdpt_cases.py) on the CPU oracle alone: conditions that keep the
GPU comparison of tests/test_gpu_bdpt_coverage.py from being vacuous.  A case whose oracle image is black, or whose
image does not depend on the thing the case is about, would pass on the device whatever the kernels did."""
import numpy as np
import pytest

import bdpt_cases as bc


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_case_is_not_vacuous(oracle_mod, name):
    case = bc.CASE_BY_NAME[name]
    args, img, st = bc.reference(oracle_mod, name)
    W, H, spp = args[5], args[6], args[9]
    assert W <= 48 and H <= 36 and spp <= 3
    assert img.shape == (H, W, 3) and np.isfinite(img).all() and img.min() >= 0.0
    lit = bc.lit_share(img)
    print("%s: lit %.3f, connections %d" % (name, lit, st["connections"]))
    if case.dark is None:
        assert lit >= 0.5, lit
    if name not in bc.EXEMPT_CONNECTIONS:
        assert st["connections"] > 0
    if name in bc.ALL_ZERO:
        assert not img.any()


def test_exemptions_are_the_named_ones():
    dark = {c.name for c in bc.CASES if c.dark}
    assert dark == {"depths-e1-l1-spl1", "nlv-l1-spl1"} | {"edge-" + e for e in bc.EDGE}
    assert all(isinstance(c.dark, str) and len(c.dark) > 10 for c in bc.CASES if c.dark)
    assert set(bc.EXEMPT_CONNECTIONS) <= dark and set(bc.ALL_ZERO) <= set(bc.EXEMPT_CONNECTIONS)


def test_depth_cases_are_unequal():
    assert len(bc.DEPTHS) == 7
    for e, l, spl in bc.DEPTHS:
        assert e != l or (e, l, spl) == (1, 1, 1)
    assert any(e > l for e, l, _ in bc.DEPTHS) and any(e < l for e, l, _ in bc.DEPTHS)
    for c in bc.DEPTHS:
        a = bc.depth_case(*c)
        assert (a[7], a[8], a[10]) == c and len(a[0]) == 4 and len(set(a[3][2].tolist())) == 2      # input.txt: 4 lights, 2 groups


def test_nlv_cases_leave_the_tile_sizes():
    nlv = [bc.n_light_vertices(bc.nlv_case(*c)) for c in bc.ODD_NLV]
    assert nlv == [ld * spl for ld, spl in bc.ODD_NLV]
    assert {1, 63, 65} <= set(nlv) and ({7, 9} & set(nlv))
    assert {1, 63} <= {n % 64 for n in nlv} and all(n % 8 != 0 for n in nlv)
    big = bc.n_light_vertices(bc.big_nlv_case())
    assert big >= 1000 and big % 8 != 0 and big % 64 != 0


@pytest.mark.parametrize("seed", bc.GROUP_SEEDS)
def test_grouping_changes_the_image(oracle_mod, seed):
    L, sp, tr, order = bc.grouped_scene(seed)
    kind, index, group = order
    # every object once; the ids are scattered and negative, the insertion order interleaves kinds and groups
    assert sorted(zip(kind.tolist(), index.tolist())) == [(0, i) for i in range(len(sp))] + [(1, i) for i in range(len(tr))]
    assert set(group.tolist()) == set(bc.GROUP_IDS)
    assert (np.diff(kind) != 0).sum() > 2 and (np.diff(group) != 0).sum() > len(bc.GROUP_IDS)
    members = {g: [(k, i) for k, i, gg in zip(kind.tolist(), index.tolist(), group.tolist()) if gg == g] for g in bc.GROUP_IDS}
    assert members[bc.SPHERE_ONLY_GROUP] == [(0, len(sp) - 1)]
    quad = [i for k, i in members[bc.QUAD_ONLY_GROUP]]
    assert [k for k, _ in members[bc.QUAD_ONLY_GROUP]] == [1, 1] and sorted(quad) == [len(tr) - 2, len(tr) - 1]
    flat = np.concatenate([tr[k][quad] for k in ("v0", "v1", "v2")])
    assert (np.ptp(flat, axis=0) == 0).sum() == 1                                  # one degenerate axis
    # the duplicates are coincident with triangles 40.. and live in other groups
    g_of_tri = {i: g for k, i, g in zip(kind.tolist(), index.tolist(), group.tolist()) if k == 1}
    first_dup = next(i for i in range(41, len(tr)) if all(np.array_equal(tr[k][i], tr[k][40]) for k in ("v0", "v1", "v2")))
    n_dup = len(tr) - 2 - first_dup
    assert n_dup >= 12
    for k in range(n_dup):
        assert all(np.array_equal(tr[c][first_dup + k], tr[c][40 + k]) for c in ("v0", "v1", "v2"))
        assert g_of_tri[first_dup + k] != g_of_tri[40 + k]
    args, img, _ = bc.reference(oracle_mod, "groups-%d" % seed)
    one = list(args); one[3] = bc.single_group(sp, tr)
    single, _ = bc.oracle_render(oracle_mod, tuple(one))
    assert not np.array_equal(img, single)


@pytest.mark.parametrize("with_cone", [False, True])
def test_the_parallel_light_arrives(oracle_mod, with_cone):
    args, img, _ = bc.reference(oracle_mod, "parallel-open-cone" if with_cone else "parallel-open")
    L = args[0]
    assert int(L[0]["is_parallel"]) == 1 and len(L) == (2 if with_cone else 1)
    off, _ = bc.oracle_render(oracle_mod, bc.parallel_case(with_cone, parallel_on=False))
    assert (img != off).any(axis=-1).mean() >= 0.5
    if not with_cone:
        assert not off.any()


def test_max_delta_changes_the_image(oracle_mod):
    default, _ = bc.oracle_render(oracle_mod, bc.max_delta_case(0))
    images = [bc.reference(oracle_mod, "max_delta-%d" % m)[1] for m in bc.MAX_DELTAS]
    for m, img in zip(bc.MAX_DELTAS, images):
        assert bc.reference(oracle_mod, "max_delta-%d" % m)[0][12] == m
        assert not np.array_equal(img, default), m
    assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[1], images[2])


def test_far_scene_is_far():
    L, sp, tr = bc.far_case()[:3]
    lo = np.minimum.reduce([tr[k].min(axis=0) for k in ("v0", "v1", "v2")])
    hi = np.maximum.reduce([tr[k].max(axis=0) for k in ("v0", "v1", "v2")])
    assert (np.minimum(np.abs(lo), np.abs(hi)) > 100).all() and (hi - lo).max() > 64
