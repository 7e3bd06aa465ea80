"""The animation sessions (anim_cases.py) on the CPU alone: conditions that keep the device comparison of
tests/test_gpu_anim_sessions.py from being vacuous.  A session that never makes a pair of calls cannot find what that pair
breaks; a step that moves nothing, or moves something no pixel shows, passes whatever the device did; a black image passes
whatever the kernels do; and a model that cannot tell a wrong implementation from the right one guards nothing -- so eight
wrong models are run over the same sessions and each must be told apart.  The numbers printed here are the ones in
anim_cases' docstring."""
import numpy as np
import pytest

import anim_cases as ac
import morph_oracle as mo
import pose_oracle as po
import skin_oracle as so

# the ordered pairs (a, b) of session P whose step b is a refusal: b is illegal in the state the walk is in after a
REFUSED_PAIRS = {("set_parts", "skin"), ("pose", "skin"), ("set_skin", "pose"), ("skin", "pose")}
A_NAMES = ac.A_NAMES


@pytest.fixture(scope="module")
def orc(oracle_mod, tmp_path_factory):
    return ac.Oracles(oracle_mod, tmp_path_factory.mktemp("anim_oracles"))


def _sessions(hpt):
    return [ac.session(n, hpt) for n in ac.NAMES]


def _pairs(session):
    """[(a, b, refused)] of the consecutive triangle-state steps, a the last accepted one."""
    out, last = [], None
    for st in session.steps:
        k = st.kw["call"] if st.kind == "refused" else st.kind
        if k not in ac.TRI_KINDS:
            continue
        if last is not None:
            out.append((last, k, st.kind == "refused"))
        if st.kind != "refused":
            last = k
    return out


def test_vocabulary(hpt):
    steps = [st for s in _sessions(hpt) for st in s.steps]
    kinds = {st.kind for st in steps}
    assert kinds == set(ac.STATE_KINDS) | set(ac.OBSERVATIONS) | {"refused"}
    assert {st.kw["walk"] for st in steps if st.kind == "pt"} == set(ac.WALKS)
    assert {st.kw["label"] for st in steps if st.kind == "refused"} == set(ac.REFUSALS)
    assert {st.kw["depth"] for st in steps if st.kind == "rebuild_device_bounded"} == set(ac.DEPTHS)
    assert {st.kw["which"] for st in steps if st.kind == "set_groups"} == set(ac.GROUPS)
    tables = {st.kw["table"] for st in steps if st.kind in ("pose", "skin")}
    assert {"identity", "nan1", "nan_all", "lift"} <= tables
    assert {st.kw["skin"] for st in steps if st.kind == "set_skin"} == set(ac.SKINS)
    assert {st.kw["morphs"] for st in steps if st.kind == "set_morphs"} == set(ac.MORPHS)
    ws = [st.kw["w"] for st in steps if st.kind == "morph"]
    assert any(ac.all_inactive(w) and np.signbit(w).any() for w in ws) and any(min(w) < 0 for w in ws) and any(np.isinf(w).any() for w in ws)
    assert any(w[1] != 0 for w in ws if len(w) == 4) and any(w[2] == 0 and any(w) for w in ws if len(w) == 4) and any(w[2] == 1 for w in ws if len(w) == 4)
    assert {s.name: len(s.steps) for s in _sessions(hpt)} == dict(P=540, K=207, M1=98, M2=98, M3=98, M4=98, F=96, T=40, Z=26, **{n: ac.A_STEPS for n in A_NAMES})


def test_p_makes_every_ordered_pair(hpt):
    p = ac.session("P", hpt)
    pairs = _pairs(p)
    assert {(a, b) for a, b, _ in pairs} == {(a, b) for a in ac.TRI_KINDS for b in ac.TRI_KINDS}
    assert len({(a, b) for a, b, _ in pairs}) == 121
    assert {(a, b) for a, b, r in pairs if r} == REFUSED_PAIRS
    # every state-changing or refused step is followed by records, tree and a pt, whose walk cycles
    walks = []
    for i, st in enumerate(p.steps):
        if ac.is_change(st):
            assert [x.kind for x in p.steps[i + 1:i + 4]] == ["records", "tree", "pt"], i
            walks.append(p.steps[i + 3].kw["walk"])
    assert walks == [ac.WALKS[i % 5] for i in range(len(walks))]
    t, z = ac.session("T", hpt), ac.session("Z", hpt)
    assert len(t.steps) == 40 and [(st.kw.get("call", st.kind)) for st in t.steps] == [(st.kw.get("call", st.kind)) for st in p.steps[:40]]
    assert {st.kind for st in z.steps} >= set(ac.STATE_KINDS) | set(ac.OBSERVATIONS)
    print("P: %d steps, %d state-changing or refused; %d pairs are refusals; T %d steps, Z %d steps"
          % (len(p.steps), sum(ac.is_change(st) for st in p.steps), len(REFUSED_PAIRS), len(t.steps), len(z.steps)))


@pytest.mark.parametrize("name", ac.NAMES)
def test_the_model_is_the_definitions(hpt, name):
    """cur after every step: hpt_morph_host composed with hpt_pose_host / hpt_skin_host, and the numpy restatements."""
    s = ac.session(name, hpt)
    for i, z in enumerate(ac.replay(hpt, s)):
        m_host = z.R if z.targets is None else hpt.morph_host(z.R, *z.targets, z.weights)
        m_np = z.R if z.targets is None else mo.morph(z.R, *z.targets, z.weights)
        if z.deformer is None or z.table is None:
            host, rest = m_host, m_np
        elif z.deformer[0] == "parts":
            host, rest = hpt.pose_host(m_host, z.deformer[1], z.table), po.pose(m_np, z.deformer[1].astype(np.int64), z.table)
        else:
            host, rest = hpt.skin_host(m_host, z.deformer[1], z.deformer[2], z.table), so.skin(m_np, z.deformer[1], z.deformer[2], z.table)
        assert z.cur.tobytes() == host.tobytes(), (name, i, s.steps[i])
        assert z.cur.tobytes() == rest.tobytes(), (name, i, s.steps[i])
        base = ac.scene(s.scene)["tr"]
        assert po.with_verts(z.cur, po.verts_of(base)).tobytes() == base.tobytes(), (name, i)         # the 84 other bytes never change


def _expected_to_stay(st):
    return (st.kind in ("refused", "set_parts", "set_skin", "set_morphs", "update_rounds", "keep_previous", "set_groups") + ac.BUILD_KINDS + ac.OBSERVATIONS
            or (st.kind in ("pose", "skin") and st.kw["table"] == "identity") or (st.kind == "morph" and ac.all_inactive(st.kw["w"])))


@pytest.mark.parametrize("name", ac.NAMES)
def test_steps_are_visible_and_images_lit(hpt, orc, name):
    s = ac.session(name, hpt)
    sd = ac.scene(s.scene)
    snaps = ac.replay(hpt, s)
    before = ac.Model(hpt, sd).snap()
    geometry = same = 0
    dark, dimmest = [], 1.0
    for i, (st, z) in enumerate(zip(s.steps, snaps)):
        moved = z.cur.tobytes() != before.cur.tobytes()
        if moved:
            assert st.kind in ac.GEOMETRY_KINDS, (name, i, st)
            a, b = ac.pt_image(orc, sd, before)[0], ac.pt_image(orc, sd, z)[0]
            assert (a.view(np.uint32) != b.view(np.uint32)).any(), "%s step %d %r moves the geometry and no pixel" % (name, i, st)
        else:
            assert _expected_to_stay(st) or s.scene == "none", "%s step %d %r leaves the geometry's bytes alone" % (name, i, st)
        if st.kind in ac.GEOMETRY_KINDS:
            geometry, same = geometry + 1, same + (not moved)
        if st.kind in ("pt", "bdpt", "ppm"):
            img = ac.observe(orc, sd, z, st)["image"]
            assert np.isfinite(img).all() and img.min() >= 0.0, (name, i, st)
            lit = float((img.sum(axis=-1) > 0).mean())
            if z.live == 0 and z.updates > 0 or s.scene == "none":
                dark.append(i)                                       # K's all-dead steps and Z: whatever the light ball alone gives
            else:
                assert lit >= 0.5, (name, i, st, lit)
                dimmest = min(dimmest, lit)
        before = z
    share = same / max(geometry, 1)
    print("%s: %d accepted geometry steps, %d byte-equal (%.2f); dimmest image lit on %.2f; all-dead or empty renders at %s"
          % (name, geometry, same, share, dimmest, dark))
    assert name in ("K", "Z") or not dark, (name, dark)              # only K's all-dead steps and Z are exempt from the lit bound
    if name[0] == "A":
        assert geometry >= 4 and share <= 0.5, (name, geometry, same)
    if name == "K":
        # every triangle dead at one point on each build kind
        dead_builds = {st.kind for st, z in zip(s.steps, snaps) if st.kind in ac.BUILD_KINDS and z.dead == sd["n"]}
        assert dead_builds == set(ac.BUILD_KINDS)
        assert {z.tree.kind for z in snaps if z.dead == sd["n"]} >= {"host", "device", "bounded"}


def _signature(hpt, orc, sd, st, z):
    sig = [("cur", z.cur.tobytes()), ("tree", ac.tree_bytes(ac.expected_tree(hpt, z.tree, z.cur)))]
    if st.kind == "guides":
        g = ac.observe(orc, sd, z, st)
        sig.append(("guide", b"".join(g[k].tobytes() for k in sorted(g))))
    return sig


def _first_difference(hpt, orc, name, mutant):
    s = ac.session(name, hpt)
    sd = ac.scene(s.scene)
    for i, (st, a, b) in enumerate(zip(s.steps, ac.replay(hpt, s), ac.replay(hpt, s, mutant))):
        for (what, x), (_, y) in zip(_signature(hpt, orc, sd, st, a), _signature(hpt, orc, sd, st, b)):
            if x != y:
                return i, what
    return None


# mutant -> (session, step, what) that first tells it apart among P, M1..M4 and F, and the random sessions that tell it apart
MUTANTS_SEEN = {
    "i": (("P", 288, "cur"), ["A1", "A2", "A3", "A4", "A5", "A6"]),
    "ii": (("P", 324, "cur"), ["A1", "A2", "A4", "A6"]),
    "iii": (("P", 56, "cur"), ["A1", "A2", "A3"]),
    "iv": (("P", 232, "cur"), ["A1", "A2", "A3", "A5"]),
    "v": (("M1", 20, "cur"), ["A4", "A6"]),
    "vi": (("P", 64, "tree"), ["A1", "A2", "A3", "A4", "A5", "A6"]),
    "vii": (("F", 22, "tree"), ["A1", "A2", "A3", "A4", "A5"]),
    "viii": (("F", 10, "guide"), ["A3", "A5"]),
}


@pytest.mark.parametrize("mutant", ac.MUTANTS)
def test_the_sessions_tell_a_wrong_model_apart(hpt, orc, mutant):
    fixed = None
    for name in ["P", "M1", "M2", "M3", "M4", "F"]:
        d = _first_difference(hpt, orc, name, mutant)
        if d is not None:
            fixed = (name,) + d
            break
    random = [n for n in A_NAMES if _first_difference(hpt, orc, n, mutant) is not None]
    print("mutant %s: first told apart by %s; random sessions %s" % (mutant, fixed, " ".join(random)))
    assert fixed is not None, mutant
    assert len(random) >= 2, (mutant, random)
    assert (fixed, random) == MUTANTS_SEEN[mutant]


def test_expected_trees(hpt):
    depths, forced, rule = [], [], 0
    for s in _sessions(hpt):
        seen = set()
        for st, z in zip(s.steps, ac.replay(hpt, s)):
            t = ac.expected_tree(hpt, z.tree, z.cur)
            depths.append(t["bvh_depth"])
            assert t["bvh_depth"] <= 30, (s.name, st)
            if z.tree.kind == "bounded":
                assert t["bvh_depth"] <= (z.tree.depth or 30), (s.name, st)
                assert t["bounded"] == z.bounded or st.kind != "rebuild_device_bounded"
            if st.kind == "rebuild_device_bounded":
                forced.append(z.bounded["forced_nodes"])
                assert z.bounded["max_depth"] == (ac.depth(ac.scene(s.scene), st.kw["depth"]) or 30)
            if z.tree.kind in ("created", "host") and id(z.tree.T) not in seen:
                # the one rule: the builder's own export of T is its refit to T
                seen.add(id(z.tree.T))
                rule += 1
                assert ac.tree_bytes(hpt.export_bvh_host(z.tree.L, z.tree.sp, z.tree.T)) == ac.tree_bytes(hpt.refit_bvh_host(z.tree.L, z.tree.sp, z.tree.T, z.tree.T)), (s.name, st)
            assert z.fell_back == 0                                  # no session's device build falls back: the model would follow it
    assert min(forced) == 0 and max(forced) > 0
    # the figures anim_cases' docstring and DESIGN.md quote
    assert (min(depths), max(depths), max(forced), len(forced), rule) == (0, 15, 116, 34, 33)
    print("trees: bvh_depth %d .. %d; forced_nodes %d .. %d over %d bounded builds; the builder's export checked against its refit for %d trees"
          % (min(depths), max(depths), min(forced), max(forced), len(forced), rule))
