"""Animation sessions on the MI355X: every session of anim_cases.py on ONE hpt.Scene from its first step to its last, held
step by step to the host model of the handle (anim_cases.Model, which restates include/hpt.h) and to the CPU oracles.

After every state-changing or refused step: read_triangles against the model's records; export_bvh against the definition of
the tree's kind built from the records at build time and refitted to the current ones; tree_cost against tree_cost_host of
that export; update_info's counts, has_motion, rebuild_info, device_build_info, bounded_build_info and the tree's size in
stats against the model.  At every observation step the image, guides or probes against the oracles' bytes; every walk of
the path tracer gives the scan's image, the counting one also the oracle's ray counts.  A refused step raises
"hpt error 1:" and leaves all of the above as it was.  Two more tests run P and A1 on twin handles: one that skips the
builds, and one that is handed the model's records through update_triangles instead of the deformer calls.

A mismatch names the session, the step and its record.  tests/test_anim_cases_cpu.py keeps the sessions' steps visible, their
images lit and the model able to tell eight wrong implementations apart."""
import numpy as np
import pytest

import anim_cases as ac
import cost_oracle as co
import pose_oracle as po
from test_gpu_refit import TREE_KEYS, _params

pytestmark = pytest.mark.gpu

U32 = np.uint32
COUNTED = ("samples", "closest_rays", "shadow_rays")
GUIDE_KEYS = ("albedo", "normal", "position", "coverage", "prev_position")


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def orc(oracle_mod, tmp_path_factory):
    return ac.Oracles(oracle_mod, tmp_path_factory.mktemp("anim_oracles"))


def _where(session, i):
    return "session %s, step %d, %s %r" % (session.name, i, session.steps[i].kind, session.steps[i].kw)


def _same(session, i, what, got, want, nan_is_nan=False):
    """Byte equality, as test_gpu_sessions._same: a mismatch names the session, the step and the first differing value.
    nan_is_nan: two NaNs of different bits pass (the motion guide's Y is not defined beyond "non-finite", include/hpt.h)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        pytest.fail("%s: %s is %s %s, expected %s %s" % (_where(session, i), what, got.dtype, got.shape, want.dtype, want.shape))
    if got.tobytes() == want.tobytes():
        return
    if got.dtype.names:                                              # records: the message names a vertex where one differs
        rows = np.nonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1))[0]
        got, want = po.verts_of(got), po.verts_of(want)
        if got.tobytes() == want.tobytes():
            pytest.fail("%s: %s differs in the non-vertex bytes of %d of %d records, first record %d"
                        % (_where(session, i), what, len(rows), len(got), int(rows[0])))
    bits = "u%d" % got.dtype.itemsize
    bad = got.view(bits) != want.view(bits)
    if nan_is_nan:
        bad &= ~(np.isnan(got) & np.isnan(want))
        if not bad.any():
            return                                                   # every difference is a NaN on both sides
    diff = np.argwhere(bad)
    at = tuple(int(v) for v in diff[0])
    pytest.fail("%s: %s differs in %d of %d values, first at %s: got %r, expected %r"
                % (_where(session, i), what, len(diff), got.size, at, got[at].item(), want[at].item()))


def _equal(session, i, what, got, want):
    assert got == want, "%s: %s is %r, expected %r" % (_where(session, i), what, got, want)


class Handle:
    """One hpt.Scene of a session's scene and the calls of the steps."""

    def __init__(self, hpt, torch, session):
        self.hpt, self.torch, self.session = hpt, torch, session
        self.sd = sd = ac.scene(session.scene)
        self.scene = hpt.Scene(sd["L"], sd["sp"], sd["tr"])

    def close(self):
        self.scene.close()

    def call(self, st):
        """The call of an accepted state-changing step."""
        sd, h, k, kw = self.sd, self.scene, st.kind, st.kw
        if k == "update_triangles":
            h.update_triangles(ac.edit(sd, kw["edit"]))
        elif k == "update_vertices_device":
            h.update_vertices_device(self.torch.from_numpy(np.ascontiguousarray(po.verts_of(ac.edit(sd, kw["edit"])))).cuda())
        elif k == "set_parts":
            h.set_parts(*ac.parts(sd))
        elif k in ("pose", "skin"):
            getattr(h, k)(ac.table(sd, kw["table"]))
        elif k == "set_skin":
            h.set_skin(*ac.skin(sd, kw["skin"]))
        elif k == "set_morphs":
            h.set_morphs(*ac.morphs(sd, kw["morphs"]))
        elif k == "morph":
            h.morph(ac.weights(kw["w"]))
        elif k == "rebuild":
            h.rebuild()
        elif k == "rebuild_device":
            h.rebuild_device()
        elif k == "rebuild_device_bounded":
            h.rebuild_device_bounded(ac.depth(sd, kw["depth"]))
        elif k == "update_rounds":
            h.update_rounds(*ac.rounds(sd, kw["edit"]))
        elif k == "keep_previous":
            h.keep_previous()
        elif k == "set_groups":
            h.set_groups(*(sd["order"] if kw["which"] == "bend" else [np.zeros(0, np.int32)] * 3))
        else:
            raise ValueError(k)

    def refused(self, i, st, model):
        method, args = ac.refused_args(self.sd, model, st.kw)
        with pytest.raises(self.hpt.HptError) as e:
            getattr(self.scene, method)(*args)
        assert str(e.value).startswith("hpt error %d:" % ac.ERR_INVALID), "%s: %s" % (_where(self.session, i), e.value)

    def observe(self, st):
        """What the device gives at an observation step: a dict of arrays (pt: also the counted rays)."""
        hpt, sd, h, k, kw = self.hpt, self.sd, self.scene, st.kind, st.kw
        if k == "pt":
            flags, budget = dict([("default", (0, 0)), ("brute force", (hpt.FLAG_BRUTE_FORCE, 0)), ("budget 1", (0, 1)), ("budget 63", (0, 63)),
                                  ("counting", (hpt.FLAG_COUNT_WORK, 0))])[kw["walk"]]
            out = dict(image=h.render_pt(ac.camera(sd), ac.W, ac.H, ac.DEPTH, ac.SPP, _params(hpt, flags, budget, seed=ac.SEED)))
            if kw["walk"] == "counting":
                stats = h.stats()
                out["counted"] = {c: int(stats[c]) for c in COUNTED}
            return out
        if k == "bdpt":
            b = ac.BDPT
            return dict(image=h.render_bdpt(ac.bdpt_camera(sd), ac.W, ac.H, b["eye_depth"], b["light_depth"], b["spp"], b["spl"], hpt.make_params(seed=b["seed"])))
        if k == "ppm":
            p = ac.PPM
            return dict(image=h.render_ppm(ac.camera(sd), ac.W, ac.H, p["eye_depth"], p["light_depth"], p["spp"], p["spl"], p["radius"],
                                           hpt.make_params(seed=p["seed"])))
        if k == "guides":
            return h.render_guides(ac.camera(sd), ac.W, ac.H, ac.SPP, hpt.make_params(seed=ac.GUIDE_SEED), prev_position=True)
        raise ValueError(k)


def _check_tree(hpt, h, session, i, z):
    dev, want = h.scene.export_bvh(), ac.expected_tree(hpt, z.tree, z.cur)
    for key in TREE_KEYS:
        _same(session, i, "exported %s (a %s tree)" % (key, z.tree.kind), dev[key], want[key])
    got, host = h.scene.tree_cost(), hpt.tree_cost_host(dev)
    co.same(_where(session, i) + ": tree cost", got, host)
    _equal(session, i, "the bytes of hpt_tree_cost", got["bytes"], host["bytes"])
    st = h.scene.stats()
    _equal(session, i, "hpt_stats.bvh_nodes, bvh_depth", (st["bvh_nodes"], st["bvh_depth"]), (dev["num_nodes"], dev["bvh_depth"]))


def _check_infos(h, session, i, z):
    info = h.scene.update_info()
    _equal(session, i, "hpt_update_info (updates, live, dead)", (info["updates"], info["live_tris"], info["dead_tris"]), (z.updates, z.live, z.dead))
    _equal(session, i, "has_motion", h.scene.has_motion(), z.motion)
    _equal(session, i, "hpt_rebuild_info.rebuilds", h.scene.rebuild_info()["rebuilds"], z.rebuilds)
    di = h.scene.device_build_info()
    _equal(session, i, "hpt_device_build_info (builds, fell_back)", (di["builds"], di["fell_back"]), (z.builds, z.fell_back))
    _equal(session, i, "hpt_bounded_build_info", h.scene.bounded_build_info(), z.bounded)


def _check_state(hpt, h, session, i, z):
    _same(session, i, "read_triangles", h.scene.read_triangles(), z.cur)
    _check_tree(hpt, h, session, i, z)
    _check_infos(h, session, i, z)


def _check_observation(hpt, orc, h, session, i, z):
    st = session.steps[i]
    k = st.kind
    if k == "tree":
        return _check_tree(hpt, h, session, i, z)
    if k == "records":
        return _same(session, i, "read_triangles", h.scene.read_triangles(), z.cur)
    if k == "infos":
        return _check_infos(h, session, i, z)
    want = ac.observe(orc, h.sd, z, st)
    if k == "probe_closest":
        o, d, _ = ac.probe_rays(z, st.kw["seed"])
        t, prim = h.scene.trace_closest(o, d)
        _same(session, i, "trace_closest prim", prim, want["prim"])
        return _same(session, i, "trace_closest t", t, want["t"])
    if k == "probe_visibility":
        o, _, p2 = ac.probe_rays(z, st.kw["seed"])
        return _same(session, i, "trace_visibility", h.scene.trace_visibility(o, p2), want["visible"])
    got = h.observe(st)
    if k == "guides":
        for key in GUIDE_KEYS:
            _same(session, i, "guide " + key, got[key], want[key], nan_is_nan=key == "prev_position")
        _equal(session, i, "the NaNs of prev_position", int(np.isnan(got["prev_position"]).sum()), int(np.isnan(want["prev_position"]).sum()))
        return
    _same(session, i, "image", got["image"], want["image"])
    if "counted" in got:
        _equal(session, i, "the counted rays", got["counted"], {c: int(want["stats"][c]) for c in COUNTED})


def _run(hpt, torch, orc, name):
    session = ac.session(name, hpt)
    snaps = ac.replay(hpt, session)
    model = ac.Model(hpt, ac.scene(session.scene))
    h = Handle(hpt, torch, session)
    try:
        for i, (st, z) in enumerate(zip(session.steps, snaps)):
            if st.kind == "refused":
                h.refused(i, st, model)
            elif st.kind in ac.STATE_KINDS:
                h.call(st)
            model.apply(st)
            if ac.is_change(st):
                _check_state(hpt, h, session, i, z)
            else:
                _check_observation(hpt, orc, h, session, i, z)
    finally:
        h.close()


def test_session_p_every_pair(hpt, torch, orc):
    _run(hpt, torch, orc, "P")


def test_session_k_killed_and_revived(hpt, torch, orc):
    _run(hpt, torch, orc, "K")


@pytest.mark.parametrize("name", ["M1", "M2", "M3", "M4"])
def test_session_m_first_allocation(hpt, torch, orc, name):
    """One handle per order: the morphed rest pose is allocated once in a handle's life."""
    _run(hpt, torch, orc, name)


def test_session_f_frames(hpt, torch, orc):
    _run(hpt, torch, orc, "F")


def test_session_t_three_triangles(hpt, torch, orc):
    _run(hpt, torch, orc, "T")


def test_session_z_no_triangles(hpt, torch, orc):
    _run(hpt, torch, orc, "Z")


@pytest.mark.parametrize("name", ac.A_NAMES)
def test_random_session(hpt, torch, orc, name):
    _run(hpt, torch, orc, name)


# ---- twins -----------------------------------------------------------------------------------------------------------------
RENDERS = ("pt", "bdpt", "ppm", "guides")


def _is_build(st):
    return st.kind in ac.BUILD_KINDS or (st.kind == "refused" and st.kw["call"] in ac.BUILD_KINDS)


def _same_renders(a, b, session, i, st, what):
    ga, gb = a.observe(st), b.observe(st)
    for key in sorted(ga):
        if isinstance(ga[key], np.ndarray):
            _same(session, i, "%s of %s" % (key, what), ga[key], gb[key])


@pytest.mark.parametrize("name", ["P", "A1"])
def test_rebuild_twins(hpt, torch, name):
    """One handle makes the builds, the other skips them; every other step is the same call.  Records, images, guides, update
    counts and motion flags agree step by step: a build of any kind changes the tree and nothing else."""
    session = ac.session(name, hpt)
    model = ac.Model(hpt, ac.scene(session.scene))
    a, b = Handle(hpt, torch, session), Handle(hpt, torch, session)
    try:
        for i, st in enumerate(session.steps):
            for h in (a, b):
                if h is b and _is_build(st):
                    continue
                if st.kind == "refused":
                    h.refused(i, st, model)
                elif st.kind in ac.STATE_KINDS:
                    h.call(st)
            model.apply(st)
            if ac.is_change(st):
                _same(session, i, "read_triangles against the twin without builds", a.scene.read_triangles(), b.scene.read_triangles())
                ia, ib = a.scene.update_info(), b.scene.update_info()
                _equal(session, i, "hpt_update_info against the twin", [ia[k] for k in ("updates", "live_tris", "dead_tris")], [ib[k] for k in ("updates", "live_tris", "dead_tris")])
                _equal(session, i, "has_motion against the twin", a.scene.has_motion(), b.scene.has_motion())
            elif st.kind in RENDERS:
                _same_renders(a, b, session, i, st, "the twin without builds")
        assert b.scene.rebuild_info()["rebuilds"] == 0 and b.scene.device_build_info()["builds"] == 0 and a.scene.device_build_info()["builds"] > 0
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["P", "A1"])
def test_deformer_twins(hpt, torch, name):
    """One handle uses the deformer calls, the other is handed the model's records through update_triangles wherever an
    accepted step moves the geometry; builds and everything else are made on both.  Images and guides agree, and both trees
    are their own definitions -- which here are one: the same records at the build, the same records now."""
    session = ac.session(name, hpt)
    snaps = ac.replay(hpt, session)
    model = ac.Model(hpt, ac.scene(session.scene))
    a, b = Handle(hpt, torch, session), Handle(hpt, torch, session)
    try:
        for i, (st, z) in enumerate(zip(session.steps, snaps)):
            if st.kind == "refused":
                a.refused(i, st, model)
            elif st.kind in ac.STATE_KINDS:
                a.call(st)
                if st.kind in ac.GEOMETRY_KINDS:
                    b.scene.update_triangles(z.cur)
                elif st.kind not in ("set_parts", "set_skin", "set_morphs"):
                    b.call(st)
            model.apply(st)
            if ac.is_change(st):
                for h, who in ((a, "the deformed handle"), (b, "the handle given records")):
                    dev, want = h.scene.export_bvh(), ac.expected_tree(hpt, z.tree, z.cur)
                    for key in TREE_KEYS:
                        _same(session, i, "exported %s of %s" % (key, who), dev[key], want[key])
            elif st.kind in RENDERS:
                _same_renders(a, b, session, i, st, "the twin given records")
    finally:
        a.close()
        b.close()
