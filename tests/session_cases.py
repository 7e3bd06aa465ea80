"""Case table of the session suite: ordered lists of calls made on ONE handle that stays alive from the first call to the
last, the way the reference's front-end uses a scene (one scene, a render every frame: another --mode, another size, a
moved camera).  Inside hpt_scene nearly everything is shared between the integrators, grows on demand and keeps no old
contents: pass[0]'s path state, queues and shadow records; its counter buffer, laid out three ways (PT 4 x (iters + 2),
BDPT 2 x (iters + 2), PPM 4 M + 2); the accumulator, the work counters, the own local framebuffer and image, the two
render events; the bidirectional tables sized by slots, slots x eye_depth, slots x n_lv and n_lv; the photon-mapping
buffers sized by n_local, deposits and buckets.  A test that opens a handle, renders once and closes it sees none of
that.  A plain module: no GPU, no tests.

A session is `Session(name, scene, handle, steps)`: scene "input" (tests/golden/scenes/input.txt: glass, mirror, four
cone lights, two groups) or "cornell2k" (cornell_with_sphere(2000): deep enough for the split trace step and the resume
launch); handle "scene" (path_tracing_amd.Scene), "multi" (MultiScene, three ranks on device 0, peer copies) or
"wrappers" (the one-shot wrappers and the scene they keep).  A step is `Step(kind, kw, repeat_of)`; repeat_of is None
or the index of an earlier step whose bytes this one must reproduce.  Kinds:

  pt, bdpt, ppm, guides        blocking renders; kw W, H, depth (eye depth), spp, seed, sample_offset, max_delta, tile,
                               samples_per_pass, flags, budget (hpt_params.reserved >> 1); bdpt and ppm also light_depth,
                               spl; ppm also radius
  pt_device_rank, untile       world = 3: one rank's tiles rendered on a side stream into row `rank` of the gathered buffer
                               named `group` (other steps may sit between the three ranks), then the assembled image
  set_groups                   which = "file" (the scene file's order) or "none" (zero objects: back to the default)
  sppm_create, sppm_render, sppm_reset, sppm_state, sppm_destroy      addressed to the state named `name`
  probe_closest, probe_visibility, export_bvh                          n seeded rays / segments; the device's tree
  stats                        hpt_get_stats after the step before it, always a blocking render (refused calls in between
                               do not count: the statistics stay the last render's)
  refused                      `call` with arguments the host rejects before it launches or allocates anything; `code` is
                               HPT_ERR_INVALID (1) or HPT_ERR_NOMEM (3)
  pt_wrapper, bdpt_wrapper, ppm_wrapper                                the one-shot calls; `changed` = one float of one
                                                                       triangle moved
  update_triangles, update_rounds                                      Scene.update_triangles / Scene.update_rounds with the
                                                                       records of the edit named `edit` (EDITS below)

Scene updates.  An edit is a named, pure function of the session scene's BASE records (never of the records in force), so
edits follow each other in any order; `base` returns to the original records.  A triangle edit replaces the triangles, a
rounds edit the lights and the spheres, and the handle holds `current(scene, triangle edit, rounds edit)`.  Everything
expected after an update is computed from those records by the same oracles: the images, photon mapping's null bounds
(ppm_oracle.scene_bounds), the probes' rays (drawn inside the live bounds), the exported tree (the runner holds it to
refit_bvh_host of the base records and the current triangles), update_info's counts after every update_triangles step.
A pt_device_rank row is the tiling of the image of the scene AT THE TIME that rank was rendered and untile assembles
those rows, so a group that straddles an update is a defined mixture.  A progressive state's records are replaced at every
update; its R2, N, tau, D and K are kept, and its bounds stay the ones it took when it was created until sppm_reset, which
takes the current scene's (every state here is created with null bounds).  So a render after an update without a reset
has an exact expected value -- old statistics, old bounds, new scene -- and a render after a reset equals a state freshly
created on the new scene.  notes(session) keeps what the CPU conditions need beside the expected results: the records and
grouping in force after every step, the images of a rank group's rows, and for a progressive render the image a state
that kept its create-time bounds through the reset would give (`stale`) and the one of a fresh state (`fresh`).

expected(orc, session) computes every step's result on the CPU with the oracles the other suites use, as they are:
oracle.pt_render and oracle.bdpt_render, tests/ppm_oracle, one tests/sppm_oracle.State per device state advanced in step,
tests/guides_oracle, oracle.closest_hits / oracle.visibility (the host scan of the probe tests), and
path_tracing_amd.tiling for a rank's packed local buffer.

Sessions (tests/test_session_cases_cpu.py holds the table to its conditions; tests/test_gpu_sessions.py runs it):
  A  "frames", input       PT, guides, BDPT, PPM, a counting PT and a PPM each followed by stats, set_groups, a PT that grows
                           every pass buffer with both pipelines in flight, a BDPT with fewer slots but more history and light
                           vertices, a 1 x 1 guide image, the default grouping again, and the first BDPT and PT steps repeated.
     A_fresh               a handle whose first render is PPM, then stats (the work counters were never written)
  B  "flags", cornell2k    one PT shape under every flag and trace budget, max_delta 250 -> 1 -> default, PPM and guides steps
                           in between, the counting PPM steps growing and shrinking cand / acc; stats after every counting step
  C  two progressive states of different size, radius, alpha and tile advanced alternately with other renders between
  D  every refusal the host makes before it touches the device, each followed by a round of every kind of render;
     at the end a counting PT render, the refusals once more, and stats that are still that render's
  E  the fan-out: three ranks on one device through grow, shrink, regroup and BDPT
  F  the one-shot wrappers: the kept scene reused by another integrator, rebuilt for a changed triangle
  R1, R2, R3               24 steps each, drawn by numpy's generator from the vocabulary and the shape lists below
  G  "a scene over time", cornell2k: a round of every integrator and two progressive states, then updates (the sphere
     turned, lowered, 20 triangles dead, the scene shrunk, base) between rounds that grow and shrink the workspace and
     run every flag; the states advanced without and with a reset; a rank group that straddles an update; set_groups
     around an update; every update refusal, then a round; at the end the builder's bytes and the first images again
  G_rounds, input          update_rounds edits (a light, the spheres) and a triangle edit between PT, BDPT, PPM and a state
  G_parallel, parallel3    refit_cases' three triangles under a parallel light: a state across an update, with and without
                           a reset -- the one scene where a state's bounds reach the image
  R4, R5, R6               as R1..R3, their vocabulary also holding the updates and their refusals

Sizes.  "Path slots" are n_local x samples in flight (PT, BDPT; photon mapping: max(n_local, photons per pass)), n_local
the packed local framebuffer ceil(tiles / world) x tile^2.  Every session but D and F has a step that is strictly
larger than everything before it and a later, strictly smaller one -- in A, B, C and R a step that is not the first; in
E the first render is the largest the issue's list allows, so there the fresh handle (nothing allocated) is what it
grows from.  A and R do the same for BDPT's light-vertex count, for the deposits of the photon-mapping family (guides:
none) and for the iteration count that sizes the counter buffer.
"""
import collections
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from path_tracing_amd import scene_io as sio, tiling              # noqa: E402
from path_tracing_amd.layouts import SPHERE                        # noqa: E402
from bdpt_cases import INPUT_TXT                                   # noqa: E402
import guides_oracle                                               # noqa: E402
import ppm_oracle                                                  # noqa: E402
import refit_cases as rc                                           # noqa: E402
import sppm_oracle                                                 # noqa: E402

# HPT_FLAG_* and the error codes of include/hpt.h (the table stays free of the package's loader)
BRUTE_FORCE, COUNT_WORK, OUTPUT_SUM, TIME_KERNELS, RUSSIAN_ROULETTE, SINGLE_PIPELINE, NO_HOST_WAIT = 1, 2, 4, 8, 16, 32, 64
ERR_INVALID, ERR_NOMEM = 1, 3
MAX_DELTA_DEFAULT, MAX_DELTA_CAP = 64, 250                          # take_params, csrc/hpt_api.cpp
WORLD = 3                                                           # ranks of the pt_device_rank steps and of session E

IMAGES = [(1, 1), (7, 3), (16, 16), (48, 40), (64, 48), (96, 64)]
TILES = [8, 32, 64]
EYE_DEPTHS = [1, 4, 12]
MAX_DELTAS = [1, 0, 250]
SPLS = [0, 8, 256]
LIGHT_DEPTHS = [1, 4]
RADII = [0.05, 0.08]
MAX_SPP = 4
BDPT_TABLE_LIMIT = 256 << 20          # bytes of slots x n_lv x 16 B a step may ask for (the host accepts up to 64 GiB)

Step = collections.namedtuple("Step", "kind kw repeat_of")
Session = collections.namedtuple("Session", "name scene handle steps")

RENDERS = ("pt", "bdpt", "ppm", "guides", "sppm_render", "pt_wrapper", "bdpt_wrapper", "ppm_wrapper", "untile")
BLOCKING = ("pt", "bdpt", "ppm", "guides", "sppm_render")           # a stats step follows one of these


def S(kind, repeat_of=None, **kw):
    return Step(kind, kw, repeat_of)


# ---- scenes and cameras ----------------------------------------------------------------------------------------------
_SCENES = {}


def scene(name):
    """dict(L, sp, tr, eye, look, up, fov, file_order, default_order, lo, hi) of a session's scene, once per process."""
    if name not in _SCENES:
        if name == "input":
            sc = sio.load_scene(INPUT_TXT)
            L, sp, tr = sio.flatten_for_pt(sc)
            d = dict(eye=tuple(sc.eye), look=tuple(sc.look_at), up=tuple(sc.view_up), fov=float(sc.fov), file_order=sio.object_order(sc))
        elif name == "cornell2k":
            L, sp, tr = sio.cornell_with_sphere(2000)
            d = dict(eye=sio.CORNELL_EYE, look=sio.CORNELL_LOOK, up=sio.CORNELL_UP, fov=50.0, file_order=sio.object_order(None, sp, tr))
        elif name == "parallel3":
            p = rc.data("parallel")
            L, sp, tr = p.L, p.sp, p.tr
            d = dict(eye=p.eye, look=p.look, up=sio.CORNELL_UP, fov=50.0, file_order=sio.object_order(None, sp, tr))
        else:
            raise KeyError(name)
        lo, hi = ppm_oracle.scene_bounds(sp, tr)
        d.update(L=L, sp=sp, tr=tr, default_order=sio.object_order(None, sp, tr), lo=lo, hi=hi)
        _SCENES[name] = d
    return _SCENES[name]


def camera(sd, W, H):
    """The camera record of the PT, PPM, SPPM and guide steps (scene_io.camera_for: 50 degrees)."""
    return sio.make_camera(sd["eye"], sd["look"], sd["up"], 50.0, W, H)


def bdpt_camera(sd, W, H):
    """The record a BDPT step hands to the device; the oracle takes eye, look_at, view_up and fov themselves."""
    return sio.make_camera(sd["eye"], sd["look"], sd["up"], sd["fov"], W, H, tan_in_float=True)


def changed_triangles(tr):
    """The wrapper session's other scene: one float of one triangle changed."""
    tr2 = tr.copy()
    v = np.array(tr2["v0"][-1], np.float32)
    v[0] += np.float32(0.25)
    tr2["v0"][-1] = v
    return tr2


def probe_rays(sd, n, seed):
    """n seeded segments inside the scene's bounds: (origins, unit directions, end points), float32."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(sd["lo"], np.float64), np.asarray(sd["hi"], np.float64)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    p2 = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = p2.astype(np.float64) - o
    d = (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    return o, d, p2


# ---- edits: the records an update step hands over --------------------------------------------------------------------
BALL = slice(rc.NWALL, None)                                        # cornell2k's tessellated sphere
BOXES = slice(12, None)                                             # input.txt's group 0 behind its twelve wall triangles


def _case_step(case):
    """The first step of a refit_cases case whose base scene is cornell2k's records."""
    def edit(tr):
        assert tr.tobytes() == rc.data(case).tr.tobytes()
        return rc.records(case, 0)[2]
    return edit


def _turned(degrees):
    """The sphere turned about an axis tilted out of the tessellation's own (refit_cases.turn_case's, by any angle)."""
    return lambda tr: rc.with_verts(tr, rc.rotate_z(rc.rotate_y(rc.verts(tr)[BALL], rc.SPHERE_C, degrees), rc.SPHERE_C, degrees), BALL)


def _boxes_moved(tr):
    """The movable part of input.txt's group 0, its two boxes, turned about their middle and lifted off the floor (the
    group's walls stay: the lights and the camera are placed by them)."""
    v = rc.verts(tr)[BOXES]
    c = v.reshape(-1, 3).mean(axis=0)
    return rc.with_verts(tr, rc.rotate_z(rc.rotate_y(v, c, 50.0), c, 35.0) + np.array((-0.2, 0.3, -0.25)), BOXES)


def _spheres_scaled(L, sp):
    """input.txt's group 1, its five spheres, scaled by 1.4 about the group's middle."""
    sp = sp.copy()
    c = np.asarray(sp["center"], np.float64)
    mid = c.mean(axis=0)
    sp["center"] = ((c - mid) * 1.4 + mid).astype(np.float32)
    sp["r"] = (np.asarray(sp["r"], np.float64) * 1.4).astype(np.float32)
    return L, sp


def _light_dimmed(L, sp):
    L = L.copy()
    pos = np.array((0.2, 0.35, 0.3), np.float32)
    L[0]["pos"] = pos; L[0]["light_ball"]["center"] = pos
    L[0]["illum"] = (0.45, 0.4, 0.3)
    return L, sp


def _spheres_moved(L, sp):
    """One sphere moved and one grown."""
    sp = sp.copy()
    sp[2]["center"] = (-0.1, 0.25, 0.2)
    sp[3]["r"] = 0.25
    return L, sp


_SAME_TR, _SAME_ROUNDS = (lambda tr: tr), (lambda L, sp: (L, sp))
EDITS = {
    "cornell2k": dict(triangles=dict(base=_SAME_TR, turn30=_turned(30.0), turn60=_turned(60.0), lowered=_case_step("there-and-back"),
                                     shrunk=_case_step("shrink"), dead20=_case_step("die-and-return")),
                      rounds=dict(base=_SAME_ROUNDS)),
    "input": dict(triangles=dict(base=_SAME_TR, boxes_moved=_boxes_moved),
                  rounds=dict(base=_SAME_ROUNDS, spheres_scaled=_spheres_scaled, light_dimmed=_light_dimmed, spheres_moved=_spheres_moved)),
    "parallel3": dict(triangles=dict(base=_SAME_TR, moved=lambda tr: rc.records("parallel", 0)[2]), rounds=dict(base=_SAME_ROUNDS)),
}
_CURRENT = {}


def live_bounds(sp, tr):
    """The bounds the probes draw their rays in: spheres +- r and the vertices of the triangles that are not dead."""
    return ppm_oracle.scene_bounds(sp, tr[~rc.dead(tr)])


def current(name, tri="base", rounds="base"):
    """scene(name) with the records a handle holds after the triangle edit `tri` and the rounds edit `rounds`, `lo` and
    `hi` the live bounds of those records, `edits` = (tri, rounds); once per process.  No edit: scene(name)'s values."""
    key = (name, tri, rounds)
    if key not in _CURRENT:
        sd = scene(name)
        L, sp = EDITS[name]["rounds"][rounds](sd["L"], sd["sp"])
        tr = EDITS[name]["triangles"][tri](sd["tr"])
        assert len(tr) == len(sd["tr"]) and len(sp) == len(sd["sp"]) and len(L) == len(sd["L"])
        lo, hi = live_bounds(sp, tr)
        _CURRENT[key] = dict(sd, name=name, L=L, sp=sp, tr=tr, lo=lo, hi=hi, edits=(tri, rounds))
    return _CURRENT[key]


def after_update(cur, st):
    """The records in force after the accepted update step `st` on a handle that held `cur`."""
    tri, rounds = cur["edits"]
    return current(cur["name"], st.kw["edit"], rounds) if st.kind == "update_triangles" else current(cur["name"], tri, st.kw["edit"])


def refused_update_args(cur, kw):
    """The arguments of a refused update step: the records in force with the one thing wrong that `bad` names."""
    L, sp, tr = cur["L"], cur["sp"], cur["tr"]
    bad, at = kw["bad"], len(tr) // 2
    if kw["call"] == "update_triangles":
        if bad == "short":
            return (tr[:-1],)
        tr = tr.copy()
        if bad == "material":
            col = tr["mtl"]["base_color"].copy(); col[at] = (0.1, 0.2, 0.3); tr["mtl"]["base_color"] = col
        else:
            ids = tr["id"].copy(); ids[at] = 99999; tr["id"] = ids
        return (tr,)
    if bad == "count":
        return (L, sp[:-1] if len(sp) else np.zeros(1, SPHERE))
    sp = sp.copy()
    rough = sp["mtl"]["roughness"].copy(); rough[1] = 0.25; sp["mtl"]["roughness"] = rough
    return (L, sp)


# ---- sizes -----------------------------------------------------------------------------------------------------------
def eff_delta(kw):
    m = kw.get("max_delta", 0)
    return MAX_DELTA_DEFAULT if m <= 0 else min(m, MAX_DELTA_CAP)


def n_local(kw, world=1):
    return tiling.tiling_dims(kw["W"], kw["H"], kw.get("tile", 0) or 32, world)[3]


def in_flight(kw):
    s = kw.get("samples_per_pass", 0)
    return min(s, kw["spp"]) if s > 0 else kw["spp"]        # at these sizes the automatic pass holds every sample


def footprints(session):
    """[(step index, dict(slots, n_local[, n_lv][, deposits], iters))] of the steps that size the shared workspace."""
    nl = len(scene(session.scene)["L"])
    world = WORLD if session.handle == "multi" else 1
    states, out = {}, []
    for i, st in enumerate(session.steps):
        k, kw = st.kind, st.kw
        if k in ("pt", "pt_device_rank", "pt_wrapper"):
            loc = n_local(kw, WORLD if k == "pt_device_rank" else world)
            out.append((i, dict(slots=loc * in_flight(kw), n_local=loc, iters=kw["depth"] + eff_delta(kw))))
        elif k in ("bdpt", "bdpt_wrapper"):
            loc = n_local(kw, world)
            out.append((i, dict(slots=loc * in_flight(kw), n_local=loc, n_lv=nl * kw["spl"] * kw["light_depth"], iters=kw["depth"] + eff_delta(kw))))
        elif k in ("ppm", "ppm_wrapper", "guides", "sppm_render"):
            z = states[kw["name"]] if k == "sppm_render" else kw
            loc = n_local(z)
            spl, ld = (0, 1) if k == "guides" else (z["spl"], z["light_depth"])
            out.append((i, dict(slots=max(loc, nl * spl), n_local=loc, deposits=nl * spl * ld, iters=max(1, ld) + eff_delta(z))))
        elif k == "sppm_create":
            states[kw["name"]] = kw
    return out


def rises_and_falls(values, from_fresh=False):
    """A value strictly larger than every earlier one -- of at least one earlier one, unless the fresh handle's nothing
    counts (from_fresh) -- and a later, strictly smaller one."""
    for i, v in enumerate(values):
        if (i > 0 or from_fresh) and v > max(values[:i], default=0) and any(w < v for w in values[i + 1:]):
            return True
    return False


def size_conditions(session):
    """{quantity: bool} of the rise-and-fall conditions this session has to meet."""
    fp = [f for _, f in footprints(session)]
    keys = ["slots", "n_local"] + (["n_lv", "deposits", "iters"] if session.name == "A" or session.name.startswith("R") else [])
    return {k: rises_and_falls([f[k] for f in fp if k in f], from_fresh=session.name == "E") for k in keys}


def bdpt_table_bytes(session):
    """The largest slots x n_lv x 16 B any step of the session makes the library reserve."""
    return max([f["slots"] * max(f["n_lv"], 1) * 16 for _, f in footprints(session) if "n_lv" in f], default=0)


# ---- statistics ------------------------------------------------------------------------------------------------------
CONSTANTS = ("bvh_nodes", "bvh_depth", "n_tris", "n_materials", "ms_bvh_build", "ms_upload")
PT_WORK = ("samples", "closest_rays", "shadow_rays", "boxes_closest", "tris_closest", "boxes_shadow", "tris_shadow", "path_iters",
           "lane_steps_closest", "wave_steps_closest", "lane_steps_shadow", "wave_steps_shadow",
           "leaf_lane_closest", "leaf_wave_closest", "leaf_lane_shadow", "leaf_wave_shadow")
BD_WORK = ("bd_pairs", "bd_survivors", "bd_shadow_rays", "bd_unoccluded", "bd_nodes", "bd_tris", "bd_spheres", "bd_group_boxes")
LAUNCHES = ("n_extend", "n_shade", "n_connect", "n_other", "n_resume")
SPLIT = ("split_budget", "traced_rays_last_pass", "long_rays_last_pass")
TIMES = ("ms_extend", "ms_shade", "ms_connect", "ms_other", "ms_resume")


def last_render(session, i):
    """The step a stats step at i describes: the one before it, a blocking render -- refused calls in between do not count."""
    at = i - 1
    while at >= 0 and session.steps[at].kind == "refused":
        at -= 1
    assert at >= 0 and session.steps[at].kind in BLOCKING, "a stats step follows a blocking render"
    return at


def expected_stats(prev, prev_expected):
    """What hpt_get_stats must report after the blocking render `prev`: dict(equal = {field: value}), exact.  ms_total
    (> 0) and the scene constants (unchanged since the handle was opened) are the runner's to check."""
    k, flags = prev.kind, prev.kw.get("flags", 0)
    eq = {}
    if k in ("ppm", "guides", "sppm_render"):
        for f in PT_WORK + BD_WORK + LAUNCHES + SPLIT + TIMES:
            eq[f] = 0
    elif k == "pt":
        for f in BD_WORK:
            eq[f] = 0
        if flags & COUNT_WORK:
            st = prev_expected["stats"]
            eq.update(samples=st["samples"], closest_rays=st["closest_rays"], shadow_rays=st["shadow_rays"], split_budget=0, long_rays_last_pass=0)
            if in_flight(prev.kw) == prev.kw["spp"]:
                # one pass: its queue counters hold every ray of the render, and iteration 0's queue is the identity over
                # the slots of the packed framebuffer (k_generate), the padding past the image edge included
                eq["traced_rays_last_pass"] = st["closest_rays"] + st["shadow_rays"] - st["samples"] + n_local(prev.kw) * prev.kw["spp"]
        else:
            for f in PT_WORK:
                eq[f] = 0
        if not flags & TIME_KERNELS:
            for f in LAUNCHES + TIMES:
                eq[f] = 0
    elif k == "bdpt":
        for f in PT_WORK + SPLIT + ("n_resume", "ms_resume"):
            eq[f] = 0
        if flags & COUNT_WORK:
            eq["bd_shadow_rays"] = prev_expected["stats"]["connections"]
        else:
            for f in BD_WORK:
                eq[f] = 0
    else:
        raise ValueError("stats after %s" % k)
    return dict(equal=eq)


# ---- expected results ------------------------------------------------------------------------------------------------
class Oracles:
    """The CPU oracles a session is computed with: `pt` the oracle package (PT, BDPT, the scans), the progressive
    photon-mapping library (which exports the PPM render too) and the guide library, built into `out_dir`."""

    def __init__(self, oracle_mod, out_dir):
        self.pt = oracle_mod
        self.sppm = sppm_oracle.build(out_dir)
        self.guides = guides_oracle.build(out_dir)


_EXPECTED = {}


def _freeze(a):
    for v in (a.values() if isinstance(a, dict) else [a]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


def _pt_image(orc, sd, kw, tr=None):
    W, H, flags = kw["W"], kw["H"], kw.get("flags", 0)
    img, st = orc.pt.pt_render(sd["L"], sd["sp"], sd["tr"] if tr is None else tr, camera(sd, W, H), W, H, kw["depth"], kw["spp"],
                               seed=kw.get("seed", 1), sample_offset=kw.get("sample_offset", 0), max_delta=eff_delta(kw),
                               output_sum=bool(flags & OUTPUT_SUM), russian_roulette=bool(flags & RUSSIAN_ROULETTE))
    return dict(image=img, stats=st)


def _bdpt_image(orc, sd, kw, order, L=None, tr=None):
    W, H = kw["W"], kw["H"]
    img, st = orc.pt.bdpt_render(sd["L"] if L is None else L, sd["sp"], sd["tr"] if tr is None else tr, order, sd["eye"], sd["look"], sd["up"],
                                 sd["fov"], W, H, kw["depth"], kw["light_depth"], kw["spp"], kw["spl"], seed=kw.get("seed", 1),
                                 max_delta=min(kw.get("max_delta", 0), MAX_DELTA_CAP))
    return dict(image=img, stats=st)


def _ppm_image(orc, sd, kw, tr=None, **bounds):
    W, H, flags = kw["W"], kw["H"], kw.get("flags", 0)
    img, st = ppm_oracle.render(orc.sppm, sd["L"], sd["sp"], sd["tr"] if tr is None else tr, camera(sd, W, H), W, H, kw["depth"], kw["light_depth"],
                                kw["spp"], kw["spl"], kw.get("radius", 0.05), seed=kw.get("seed", 1), sample_offset=kw.get("sample_offset", 0),
                                max_delta=min(kw.get("max_delta", 0), MAX_DELTA_CAP), output_sum=bool(flags & OUTPUT_SUM),
                                want_work=bool(flags & COUNT_WORK), **bounds)
    return dict(image=img, stats=st)


WITNESSES = ("pt", "bdpt", "ppm", "guides")                         # the renders render_step() computes on any records
UPDATES = ("update_triangles", "update_rounds")
_NOTES = {}


def render_step(orc, cur, st, order):
    """The expected result of the render step `st` (one of WITNESSES) on the records `cur` grouped by `order`."""
    k, kw = st.kind, st.kw
    if k == "pt":
        return _pt_image(orc, cur, kw)
    if k == "bdpt":
        return _bdpt_image(orc, cur, kw, order)
    if k == "ppm":
        return _ppm_image(orc, cur, kw)
    g, hp = guides_oracle.render(orc.guides, cur["L"], cur["sp"], cur["tr"], camera(cur, kw["W"], kw["H"]), kw["W"], kw["H"], kw["spp"],
                                 seed=kw.get("seed", 1), sample_offset=kw.get("sample_offset", 0), max_delta=min(kw.get("max_delta", 0), MAX_DELTA_CAP))
    return dict(g, image=g["albedo"], hit_points=sum(hp))


def new_state(orc, cur, kw, **bounds):
    """The oracle's progressive state of an sppm_create step on the records `cur` (bounds: the scene's unless given)."""
    return sppm_oracle.State(orc.sppm, cur["L"], cur["sp"], cur["tr"], camera(cur, kw["W"], kw["H"]), kw["W"], kw["H"], kw["depth"],
                             kw["light_depth"], kw["spl"], kw["radius"], kw["alpha"], kw.get("seed", 1),
                             kw.get("sample_offset", 0), eff_delta(kw), **bounds)


def expected(orc, session):
    """The expected result of every step of the session, in order, computed once per process and shared (read-only):
    renders dict(image, stats) (guides: the four images and `hit_points`), pt_device_rank dict(local), sppm_state
    dict(radius2, photons, passes), probes dict(t, prim) / dict(visible), stats expected_stats(), refused dict(code),
    update_triangles dict(updates, live_tris, dead_tris); None for the steps that return nothing to compare (export_bvh
    is held to the host-built tree by the runner)."""
    if session.name in _EXPECTED:
        return _EXPECTED[session.name]
    sd = cur = current(session.scene)
    order, states, rank_images, rows, out, notes = sd["default_order"], {}, {}, {}, [], []
    n_updates = 0
    for i, st in enumerate(session.steps):
        k, kw, e, note = st.kind, st.kw, None, {}
        if k in WITNESSES:
            e = render_step(orc, cur, st, order)
        elif k == "pt_device_rank":
            key = (tuple(sorted((a, b) for a, b in kw.items() if a != "rank")), cur["edits"])
            if key not in rank_images:
                rank_images[key] = _pt_image(orc, cur, kw)["image"]
            rows.setdefault(kw["group"], []).append(rank_images[key])
            e = dict(local=tiling.tile_image(rank_images[key], kw.get("tile", 0) or 32, kw["rank"], WORLD))
        elif k == "untile":
            tile, images = kw.get("tile", 0) or 32, rows.pop(kw["group"])
            e = dict(image=tiling.untile_image(np.stack([tiling.tile_image(img, tile, r, WORLD) for r, img in enumerate(images)]), kw["W"], kw["H"], tile, WORLD))
            note = dict(rows=images)
        elif k == "set_groups":
            order = sd["file_order"] if kw["which"] == "file" else sd["default_order"]
        elif k in UPDATES:
            cur = after_update(cur, st)
            for z in states.values():
                for s in (z["state"], z["shadow"]):
                    if s is not None:
                        s.lights, s.spheres, s.tris = (np.ascontiguousarray(a) for a in (cur["L"], cur["sp"], cur["tr"]))
                z["updated"] = True
            if k == "update_triangles":
                n_updates += 1
                n_dead = int(rc.dead(cur["tr"]).sum())
                e = dict(updates=n_updates, live_tris=len(cur["tr"]) - n_dead, dead_tris=n_dead)
        elif k == "sppm_create":
            states[kw["name"]] = dict(state=new_state(orc, cur, kw), shadow=None, updated=False, kw=kw)
        elif k == "sppm_render":
            z = states[kw["name"]]
            img, stt = z["state"].render(kw["passes"])
            e = dict(image=img, stats=stt)
            if z["shadow"] is not None:
                note["stale"] = z["shadow"].render(kw["passes"])[0]
            if z["updated"]:
                note["fresh"] = new_state(orc, cur, z["kw"]).render(kw["passes"])[0]
        elif k == "sppm_reset":
            z = states[kw["name"]]
            if z["shadow"] is not None:
                z["shadow"].reset()
            elif z["updated"]:
                # what a reset that left the bounds alone would give from here on: the state's bounds so far, the new scene
                z["shadow"] = new_state(orc, cur, z["kw"], scene_min=z["state"].mn, scene_max=z["state"].mx)
            z["state"].reset()
            mn, mx = ppm_oracle.scene_bounds(np.ascontiguousarray(cur["sp"]), np.ascontiguousarray(cur["tr"]))
            z["state"].mn, z["state"].mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
            z["updated"] = False
        elif k == "sppm_state":
            z = states[kw["name"]]["state"]
            e = dict(radius2=z.r2.copy(), photons=z.n.copy(), passes=z.passes)
        elif k == "sppm_destroy":
            del states[kw["name"]]
        elif k == "probe_closest":
            o, d, _ = probe_rays(cur, kw["n"], kw["seed"])
            t, prim = orc.pt.closest_hits(cur["L"], cur["sp"], cur["tr"], o, d)
            e = dict(t=t, prim=prim)
        elif k == "probe_visibility":
            o, _, p2 = probe_rays(cur, kw["n"], kw["seed"])
            e = dict(visible=orc.pt.visibility(cur["sp"], cur["tr"], o, p2))
        elif k == "stats":
            at = last_render(session, i)
            e = expected_stats(session.steps[at], out[at])
        elif k == "refused":
            e = dict(code=kw["code"])
        elif k == "pt_wrapper":
            e = _pt_image(orc, sd, kw, tr=changed_triangles(sd["tr"]) if kw.get("changed") else None)
        elif k == "bdpt_wrapper":
            e = _bdpt_image(orc, sd, kw, sd["default_order"])
        elif k == "ppm_wrapper":
            e = _ppm_image(orc, sd, dict(kw, spp=1), scene_min=sd["lo"], scene_max=sd["hi"])
        elif k != "export_bvh":
            raise ValueError(k)
        out.append(_freeze(e) if e is not None else None)
        notes.append(dict(note, cur=cur, order=order))
    _EXPECTED[session.name], _NOTES[session.name] = out, notes
    return out


def notes(orc, session):
    """Per step, beside expected(): `cur` and `order`, the records (current()) and the grouping in force after the step;
    an untile step's `rows`, the images its three ranks were rows of; a progressive render's `stale` (the image of a state
    that went through the same calls but kept its bounds at every reset: present after a reset that followed an update)
    and `fresh` (the image of a state created on the current scene and advanced by as many passes: present while an
    update has not been followed by a reset)."""
    expected(orc, session)
    return _NOTES[session.name]


def result_bytes(e):
    """The bytes two steps' results are compared by (the step-must-differ condition): every array of the result."""
    return b"".join(np.ascontiguousarray(e[k]).tobytes() for k in sorted(e) if isinstance(e[k], np.ndarray))


# ---- the fixed sessions ----------------------------------------------------------------------------------------------
def _session_a():
    pt0 = dict(W=48, H=40, depth=4, spp=2, samples_per_pass=1, seed=3)                       # 4096 slots, two pipelines
    bd0 = dict(W=32, H=24, depth=4, light_depth=1, spp=2, spl=8, seed=5)                     # 2048 slots, 8192 history entries, n_lv 32
    return Session("A", "input", "scene", [
        S("pt", **pt0),
        S("guides", W=48, H=40, spp=2, seed=4),
        S("bdpt", **bd0),
        S("ppm", W=64, H=48, depth=4, light_depth=4, spp=1, spl=256, radius=0.05, seed=6),
        S("pt", W=7, H=3, depth=4, spp=4, seed=7, max_delta=1, flags=COUNT_WORK),
        S("stats"),
        S("ppm", W=16, H=16, depth=4, light_depth=1, spp=2, spl=8, radius=0.08, seed=8),
        S("stats"),                                                                          # not the counting PT step's samples
        S("set_groups", which="file"),
        S("bdpt", **dict(bd0, seed=9)),
        S("pt", W=96, H=64, depth=4, spp=4, tile=8, samples_per_pass=1, seed=10),            # 6144 slots on both pipelines
        S("bdpt", W=16, H=16, depth=12, light_depth=4, spp=4, spl=8, tile=16, seed=11),      # 1024 slots, 12288 history entries, n_lv 128
        S("guides", W=1, H=1, spp=4, seed=12),
        S("set_groups", which="none"),
        S("bdpt", repeat_of=2, **bd0),
        S("pt", repeat_of=0, **pt0),
        S("stats"),
    ])


def _session_a_fresh():
    return Session("A_fresh", "input", "scene", [
        S("ppm", W=16, H=16, depth=4, light_depth=4, spp=1, spl=8, radius=0.05, seed=13),
        S("stats"),
    ])


def _session_b():
    def pt(i, **more):
        return S("pt", **dict(dict(W=64, H=48, depth=4, spp=4, samples_per_pass=1, seed=20 + i), **more))      # 4096 slots per pipeline

    def ppm(i, W, H, flags=0, **more):
        return S("ppm", **dict(dict(W=W, H=H, depth=4, light_depth=4, spp=1, spl=256, radius=0.05, seed=40 + i, flags=flags), **more))
    return Session("B", "cornell2k", "scene", [
        pt(0, max_delta=250),
        S("guides", W=48, H=40, spp=2, seed=60, flags=TIME_KERNELS),
        pt(1, max_delta=250, flags=BRUTE_FORCE),
        ppm(0, 16, 16, COUNT_WORK), S("stats"),
        pt(2, max_delta=1, flags=COUNT_WORK), S("stats"),
        ppm(1, 96, 64, COUNT_WORK, tile=64), S("stats"),                                     # cand / acc grow: 8192 local pixels
        pt(3, max_delta=1, flags=RUSSIAN_ROULETTE),
        ppm(2, 48, 40), S("stats"),
        pt(4, flags=SINGLE_PIPELINE),
        ppm(3, 7, 3, COUNT_WORK | TIME_KERNELS, tile=8), S("stats"),                         # and shrink: 64
        pt(5, flags=NO_HOST_WAIT),
        S("guides", W=16, H=16, spp=4, seed=61), S("stats"),
        pt(6, flags=TIME_KERNELS), S("stats"),
        ppm(4, 64, 48, TIME_KERNELS, spl=8, max_delta=250),
        pt(7, flags=OUTPUT_SUM),
        S("guides", W=64, H=48, spp=1, seed=62, max_delta=1),
        pt(8, budget=1),
        ppm(5, 16, 16, spl=8),
        pt(9, budget=63),
    ])


def _session_c():
    z1 = dict(name="Z1", W=48, H=48, depth=4, light_depth=4, spl=256, radius=0.05, alpha=0.7, seed=71)
    z2 = dict(name="Z2", W=40, H=24, depth=4, light_depth=4, spl=8, radius=0.08, alpha=0.5, tile=8, seed=72)
    steps, first = [S("sppm_create", **z1), S("sppm_create", **z2)], {}

    def advance(name, passes, again=False, stats=False, **more):
        """render, [stats,] state; `again`: the steps that advanced Z1 by as many passes the first time are repeated."""
        if not again:
            first.setdefault((name, passes), len(steps))
        at = first[(name, passes)] if again else None
        steps.append(S("sppm_render", repeat_of=at, name=name, passes=passes, **more))
        if stats:
            steps.append(S("stats"))
        steps.append(S("sppm_state", repeat_of=at + 1 if again else None, name=name))

    advance("Z1", 1)
    steps.append(S("pt", W=96, H=64, depth=4, spp=2, seed=73, flags=COUNT_WORK))      # 6144 local pixels: past both states' 4096
    advance("Z2", 2, stats=True)                                                      # not the counting PT step's rays
    advance("Z1", 2)
    steps.append(S("ppm", W=16, H=16, depth=4, light_depth=4, spp=1, spl=256, radius=0.13, seed=74))
    advance("Z2", 1)
    steps.append(S("guides", W=7, H=3, spp=3, seed=75))
    steps += [S("sppm_reset", name="Z1"), S("sppm_state", name="Z1")]
    advance("Z1", 1, again=True)
    advance("Z2", 1, flags=COUNT_WORK)
    advance("Z1", 2, again=True)
    steps.append(S("sppm_destroy", name="Z2"))
    steps.append(S("pt", W=16, H=16, depth=4, spp=2, seed=76))
    advance("Z1", 1, flags=COUNT_WORK)
    return Session("C", "input", "scene", steps)


REFUSALS = [
    # label, call, what differs from the valid call of that kind, code
    ("tile 12", "pt", dict(tile=12), ERR_INVALID),
    ("eye_depth 0", "pt", dict(depth=0), ERR_INVALID),
    ("eye_depth 256", "bdpt", dict(depth=256), ERR_INVALID),
    ("spp 0", "ppm", dict(spp=0), ERR_INVALID),
    ("unknown flag bit", "pt", dict(flags=1 << 7), ERR_INVALID),
    ("reserved bit 0", "bdpt", dict(reserved=1), ERR_INVALID),
    ("world 2, PT", "pt", dict(world=2), ERR_INVALID),
    ("world 2, BDPT", "bdpt", dict(world=2), ERR_INVALID),
    ("world 2, PPM", "ppm", dict(world=2), ERR_INVALID),
    ("world 2, guides", "guides", dict(world=2), ERR_INVALID),
    ("BDPT spl 0", "bdpt", dict(spl=0), ERR_INVALID),
    ("BDPT light vertices > 2^24", "bdpt", dict(spl=(1 << 22) + 1, light_depth=1), ERR_INVALID),
    ("PPM deposits > 2^30", "ppm", dict(spl=(1 << 28) + 1, light_depth=1), ERR_NOMEM),         # the size check, not the allocator
    ("guides, every output null", "guides_null", dict(), ERR_INVALID),
    ("sppm.render(0)", "sppm_render", dict(passes=0), ERR_INVALID),
    ("sppm_create alpha 1.5", "sppm_create", dict(alpha=1.5), ERR_INVALID),
]
# the valid call of each kind that a refusal is a variation of (session D renders exactly these sizes before any refusal,
# so that no refused call finds a buffer it would have to grow on its way to the check that stops it)
VALID = dict(
    pt=dict(W=24, H=16, depth=4, spp=2),
    bdpt=dict(W=24, H=16, depth=4, light_depth=4, spp=2, spl=8),
    ppm=dict(W=24, H=16, depth=4, light_depth=4, spp=1, spl=8, radius=0.05),
    guides=dict(W=24, H=16, spp=2),
    guides_null=dict(W=24, H=16, spp=2),
    sppm_create=dict(name="bad", W=24, H=16, depth=4, light_depth=4, spl=8, radius=0.05, alpha=0.7),
    sppm_render=dict(name="Z", passes=1),
    update_triangles=dict(), update_rounds=dict(),
)
# The refusals of the scene updates: the records in force with one thing wrong (refused_update_args).  A list of its own
# because session D is REFUSALS entry by entry, on a scene that is never updated; G and G_rounds make these, each on the
# scene that can (cornell2k has no sphere whose material could change).
UPDATE_REFUSALS = [
    ("update, one record short", "update_triangles", dict(bad="short"), ERR_INVALID),
    ("update, a material byte changed", "update_triangles", dict(bad="material"), ERR_INVALID),
    ("update, an id changed", "update_triangles", dict(bad="id"), ERR_INVALID),
    ("update, another sphere count", "update_rounds", dict(bad="count"), ERR_INVALID),
    ("update, a sphere's material changed", "update_rounds", dict(bad="material"), ERR_INVALID),
]


def update_refusals(scene_name):
    """The labels of UPDATE_REFUSALS that can be made on the scene."""
    return [r[0] for r in UPDATE_REFUSALS if len(scene(scene_name)["sp"]) >= 2 or r[2] != dict(bad="material") or r[1] != "update_rounds"]


def refusal(label):
    lab, call, diff, code = next(r for r in REFUSALS + UPDATE_REFUSALS if r[0] == label)
    return S("refused", label=lab, call=call, code=code, **dict(VALID[call], **diff))


def _round(r):
    """One valid render of every kind (seeds of their own: no two rounds give the same bytes), the progressive state
    advanced by one pass and read."""
    return [S("pt", seed=100 + r, **VALID["pt"]), S("bdpt", seed=200 + r, **VALID["bdpt"]), S("ppm", seed=300 + r, **VALID["ppm"]),
            S("guides", seed=400 + r, **VALID["guides"]), S("sppm_render", name="Z", passes=1), S("sppm_state", name="Z")]


def _session_d():
    steps = [S("sppm_create", name="Z", W=24, H=16, depth=4, light_depth=4, spl=8, radius=0.05, alpha=0.7, seed=81)] + _round(0)
    for r, (label, call, _, _) in enumerate(REFUSALS, 1):
        steps.append(refusal(label))
        if call == "sppm_render":
            steps.append(S("sppm_state", name="Z"))                 # K unchanged by passes = 0
        steps += _round(r)
    # and the statistics of the last render are still its own after calls that were refused
    steps += [S("pt", seed=500, flags=COUNT_WORK, **VALID["pt"])] + [refusal(r[0]) for r in REFUSALS] + [S("stats")]
    return Session("D", "input", "scene", steps)


def _session_e():
    big = dict(W=200, H=136, depth=4, spp=2, seed=91)
    return Session("E", "input", "multi", [
        S("pt", **big),
        S("pt", W=24, H=16, depth=4, spp=2, tile=32, seed=92),                       # one tile: two ranks have none
        S("pt", W=96, H=64, depth=4, spp=2, tile=8, seed=93),
        S("set_groups", which="file"),
        S("bdpt", W=48, H=40, depth=4, light_depth=4, spp=2, spl=8, seed=94),
        S("pt", repeat_of=0, **big),
    ])


def _session_f():
    a = dict(W=48, H=40, depth=4, spp=2, seed=95)
    return Session("F", "input", "wrappers", [
        S("pt_wrapper", **a),
        S("bdpt_wrapper", W=32, H=24, depth=4, light_depth=4, spp=2, spl=8, light_sample=1, seed=96),     # the same light bytes
        S("ppm_wrapper", W=32, H=24, depth=4, light_depth=4, spl=256, seed=97),
        S("pt_wrapper", W=16, H=16, depth=4, spp=3, seed=98),
        S("pt_wrapper", changed=True, **a),
        S("pt_wrapper", repeat_of=0, **a),
    ])


def _session_g():
    pt0 = dict(W=48, H=40, depth=4, spp=2, tile=8, seed=600)                                 # 1920 local pixels, 3840 slots
    bd0 = dict(W=24, H=16, depth=4, light_depth=4, spp=2, spl=8, seed=601)
    ppm0 = dict(W=48, H=40, depth=4, light_depth=4, spp=1, spl=256, radius=0.05, tile=8, seed=602)
    gd0 = dict(W=48, H=40, spp=2, seed=603)
    z1 = dict(name="Z1", W=48, H=40, depth=4, light_depth=4, spl=256, radius=0.05, alpha=0.7, seed=604)
    z2 = dict(name="Z2", W=40, H=24, depth=4, light_depth=4, spl=256, radius=0.08, alpha=0.5, tile=8, seed=605)
    small = dict(W=16, H=16, depth=4, spp=4)
    rank = dict(group="G1", W=64, H=48, depth=4, spp=2, tile=8, seed=640)                     # 48 tiles: 16 per rank
    steps = [
        S("set_groups", which="file"),
        S("pt", **pt0), S("bdpt", **bd0), S("ppm", **ppm0), S("guides", **gd0),               # 1 .. 4: the base round
        S("sppm_create", **z1), S("sppm_create", **z2),
        S("sppm_render", name="Z1", passes=1), S("sppm_render", name="Z2", passes=1),
        S("update_triangles", edit="turn30"),
        # the round again, larger: 8192 local pixels on each of two pipelines
        S("pt", W=96, H=64, depth=4, spp=2, tile=64, samples_per_pass=1, seed=610, flags=TIME_KERNELS),
        S("bdpt", **dict(bd0, W=48, H=40, tile=8, seed=611)),
        S("ppm", **dict(ppm0, W=64, H=48, tile=64, max_delta=250, seed=612)),
        S("guides", **dict(gd0, W=64, H=48, seed=613)),
        S("sppm_render", name="Z1", passes=1), S("sppm_render", name="Z2", passes=1),         # no reset: old statistics, new scene
        S("sppm_reset", name="Z1"), S("sppm_reset", name="Z2"),
        S("sppm_render", name="Z1", passes=1), S("sppm_state", name="Z1"),
        S("sppm_render", name="Z2", passes=1), S("sppm_state", name="Z2"),
        S("update_triangles", edit="lowered"),
        # a smaller round under the flags no refitted tree has been walked with
        S("pt", seed=620, max_delta=1, flags=RUSSIAN_ROULETTE, **small),
        S("pt", seed=621, flags=SINGLE_PIPELINE, budget=1, **small),
        S("pt", seed=622, flags=OUTPUT_SUM, **small),
        S("bdpt", **dict(bd0, W=16, H=16, max_delta=1, seed=623)),
        S("ppm", **dict(ppm0, W=16, H=16, tile=32, flags=OUTPUT_SUM, seed=624)),
        S("guides", W=16, H=16, spp=4, seed=625, max_delta=1, flags=TIME_KERNELS),
        S("pt", **dict(pt0, seed=630, flags=COUNT_WORK)), S("stats"),
        S("ppm", **dict(ppm0, seed=631, flags=COUNT_WORK)), S("stats"),
        # one gathered image, an update on the null stream between its ranks
        S("pt_device_rank", rank=0, **rank),
        S("update_triangles", edit="dead20"),
        S("pt_device_rank", rank=1, **rank),
        S("pt_device_rank", rank=2, **dict(rank, flags=NO_HOST_WAIT)),
        S("untile", **rank),
        S("set_groups", which="none"), S("bdpt", **dict(bd0, seed=641)),
        S("update_triangles", edit="shrunk"),
        S("set_groups", which="file"), S("bdpt", **dict(bd0, seed=642)),
        S("probe_closest", n=257, seed=643), S("probe_visibility", n=257, seed=644),
    ]
    steps += [refusal(label) for label in update_refusals("cornell2k")]
    steps += [S("pt", **dict(pt0, seed=650)), S("bdpt", **dict(bd0, seed=651)), S("ppm", **dict(ppm0, seed=652)), S("guides", **dict(gd0, seed=653)),
              S("sppm_render", name="Z1", passes=1), S("export_bvh")]
    steps += [S("update_triangles", edit="base"), S("export_bvh"), S("pt", repeat_of=1, **pt0), S("bdpt", repeat_of=2, **bd0), S("stats")]
    return Session("G", "cornell2k", "scene", steps)


def _session_g_rounds():
    pt0 = dict(W=48, H=40, depth=4, spp=2, seed=700)
    bd0 = dict(W=32, H=24, depth=4, light_depth=4, spp=2, spl=8, seed=701)
    ppm0 = dict(W=48, H=40, depth=4, light_depth=4, spp=1, spl=256, radius=0.05, seed=702)
    steps = [
        S("pt", **pt0), S("bdpt", **bd0), S("ppm", **ppm0),
        S("sppm_create", name="Z", W=48, H=40, depth=4, light_depth=4, spl=256, radius=0.05, alpha=0.7, seed=703),
        S("sppm_render", name="Z", passes=1),
        S("update_rounds", edit="light_dimmed"),
        S("pt", **dict(pt0, seed=710)), S("bdpt", **dict(bd0, seed=711)), S("sppm_render", name="Z", passes=1),
        S("update_triangles", edit="boxes_moved"),
        S("ppm", **dict(ppm0, seed=720)), S("export_bvh"),
        S("update_rounds", edit="spheres_scaled"),
        S("guides", W=48, H=40, spp=2, seed=730), S("probe_closest", n=257, seed=731), S("probe_visibility", n=257, seed=732),
    ]
    steps += [refusal(label) for label in update_refusals("input") if "sphere" in label]
    steps += [S("pt", **dict(pt0, seed=740)), S("bdpt", **dict(bd0, seed=741)), S("ppm", **dict(ppm0, seed=742)), S("export_bvh")]
    steps += [
        S("update_rounds", edit="spheres_moved"),
        S("pt", **dict(pt0, seed=750)), S("sppm_reset", name="Z"), S("sppm_render", name="Z", passes=2), S("sppm_state", name="Z"),
        S("update_rounds", edit="base"), S("bdpt", **dict(bd0, seed=760)),
        S("update_triangles", edit="base"), S("pt", repeat_of=0, **pt0), S("stats"),
    ]
    return Session("G_rounds", "input", "scene", steps)


def _session_g_parallel():
    z = dict(name="Z", W=rc.W, H=rc.H, depth=rc.PPM["eye_depth"], light_depth=rc.PPM["light_depth"], spl=rc.PPM["spl"], radius=rc.PPM["radius"],
             alpha=0.7, seed=rc.PPM["seed"])
    ppm = dict(W=rc.W, H=rc.H, depth=4, light_depth=4, spp=1, spl=rc.PPM["spl"], radius=0.05)
    return Session("G_parallel", "parallel3", "scene", [
        S("sppm_create", **z),
        S("sppm_render", name="Z", passes=2),
        S("update_triangles", edit="moved"),
        S("sppm_render", name="Z", passes=1),                      # the bounds of the base scene, its statistics, the new triangles
        S("sppm_reset", name="Z"),
        S("sppm_render", name="Z", passes=2),                      # a state freshly created on the new scene
        S("sppm_state", name="Z"),
        S("ppm", seed=5, **ppm),
        S("update_triangles", edit="base"),
        S("sppm_reset", name="Z"),
        S("sppm_render", repeat_of=1, name="Z", passes=2),
        S("ppm", seed=6, **ppm),
    ])


# ---- the random sessions ---------------------------------------------------------------------------------------------
R_SEEDS = [1, 2, 3, 4, 5, 6]
R_UPDATING = 4                         # from this seed on the vocabulary holds the scene updates and their refusals
R_STEPS = 24
R_SCENES = {1: "input", 2: "cornell2k", 3: "input", 4: "cornell2k", 5: "input", 6: "input"}
# draws whose oracle results miss a condition only the oracles can see (a black image, two equal results): none so far.
# tests/test_session_cases_cpu.py asserts those conditions for the steps random_session() returns; an attempt that
# misses them is listed here by number and skipped, so the steps stay a function of the seed alone.
R_REJECTED = {1: (), 2: (), 3: (), 4: (), 5: (), 6: ()}
# refusals made before the call looks at the scene at all, whatever was rendered before
R_REFUSALS = ("tile 12", "spp 0", "world 2, PT", "world 2, BDPT", "world 2, PPM", "world 2, guides", "guides, every output null",
              "sppm_create alpha 1.5")
_PT_FLAGS = [0, 0, BRUTE_FORCE, COUNT_WORK, RUSSIAN_ROULETTE, SINGLE_PIPELINE, NO_HOST_WAIT, TIME_KERNELS, OUTPUT_SUM]
_PPM_FLAGS = [0, 0, COUNT_WORK, TIME_KERNELS, COUNT_WORK | TIME_KERNELS, OUTPUT_SUM]


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _draw(seed, attempt):
    """24 steps drawn in order; what may follow what (a state must be alive to be advanced, ranks come in order, stats
    follow a blocking render) is decided by the steps drawn so far."""
    rng = np.random.default_rng([seed, attempt])
    name = R_SCENES[seed]
    cornell = name == "cornell2k"
    steps, alive, group, n_groups = [], {}, None, 0
    # seeds from R_UPDATING on: the edits in force, and whether the last update still waits for the render that shows it
    updating, edits, unseen, showing = seed >= R_UPDATING, dict(update_triangles="base", update_rounds="base"), False, False

    def shape(images=IMAGES, big=False):
        # 256 pixels at least: a share of them can be seen to change (and, big: cornell2k's BDPT and guide images of a
        # few pixels are black more often than three rejected draws a seed allow)
        if showing or big:
            images = [im for im in images if im[0] * im[1] >= 256]
        W, H = _pick(rng, images)
        kw = dict(W=W, H=H, tile=_pick(rng, TILES), max_delta=_pick(rng, MAX_DELTAS), seed=1000 * seed + 10 * len(steps) + attempt % 10)
        return kw, W * H < 64

    def render_pt():
        kw, tiny = shape()
        kw.update(depth=_pick(rng, EYE_DEPTHS[1:] if tiny else EYE_DEPTHS), spp=MAX_SPP if tiny else int(rng.integers(1, MAX_SPP + 1)),
                  samples_per_pass=_pick(rng, [1, 2]), sample_offset=int(rng.integers(0, 3)))
        return kw

    for _ in range(R_STEPS):
        prev = steps[-1].kind if steps else None
        options = ["pt", "pt", "bdpt", "bdpt", "ppm", "ppm", "guides", "probe_closest", "probe_visibility", "export_bvh", "refused"]
        options += ["pt_device_rank"] * 2 if group is None or group["rank"] < WORLD else ["untile"] * 3
        if prev in BLOCKING:
            options += ["stats"] * 3
        if not cornell:
            options.append("set_groups")
        options += ["sppm_create"] if len(alive) < 2 else []
        options += ["sppm_render", "sppm_render", "sppm_state", "sppm_reset", "sppm_destroy"] if alive else []
        if updating:
            # an update is followed at once by a render that can show it; no edit is drawn while it is in force
            options = ["pt", "bdpt"] if unseen else options + [u for u in UPDATES if len(EDITS[name][u[7:]]) > 1 for _ in range(2)]
            showing, unseen = unseen, False
        k = _pick(rng, options)
        if k in UPDATES:
            edits[k] = _pick(rng, [e for e in sorted(EDITS[name][k[7:]]) if e != edits[k]])
            steps.append(S(k, edit=edits[k]))
            unseen = True
        elif k == "pt":
            steps.append(S("pt", flags=_pick(rng, _PT_FLAGS), budget=_pick(rng, [0, 0, 1, 63]), **render_pt()))
        elif k == "pt_device_rank":
            if group is None or group["rank"] >= WORLD:
                n_groups += 1
                group = dict(rank=0, kw=dict(render_pt(), group="G%d" % n_groups))
            steps.append(S("pt_device_rank", rank=group["rank"], **group["kw"]))
            group["rank"] += 1
        elif k == "untile":
            steps.append(S("untile", **group["kw"]))
            group = None
        elif k == "bdpt":
            kw, tiny = shape(IMAGES[:3] if cornell else IMAGES[:4], big=updating and cornell)
            small = kw["W"] * kw["H"] <= 256 and kw["tile"] != 64
            kw.update(depth=_pick(rng, EYE_DEPTHS[1:] if tiny else EYE_DEPTHS), light_depth=_pick(rng, LIGHT_DEPTHS),
                      spp=2 if tiny else int(rng.integers(1, 3)), samples_per_pass=_pick(rng, [0, 1]),
                      spl=_pick(rng, SPLS[1:] if small and not cornell else SPLS[1:2]), flags=_pick(rng, [0, 0, COUNT_WORK, NO_HOST_WAIT]))
            steps.append(S("bdpt", **kw))
        elif k == "ppm":
            kw, tiny = shape(IMAGES[1:])                 # (a 1 x 1 image of hit points finds no photon on either scene)
            kw.update(depth=4, light_depth=_pick(rng, LIGHT_DEPTHS[1:] if tiny else LIGHT_DEPTHS), spp=2 if tiny else int(rng.integers(1, 3)),
                      radius=_pick(rng, RADII), flags=_pick(rng, _PPM_FLAGS), sample_offset=int(rng.integers(0, 3)),
                      spl=_pick(rng, SPLS[2:] if tiny else SPLS[1:] if kw["W"] * kw["H"] < 48 * 40 else SPLS))
            steps.append(S("ppm", **kw))
        elif k == "guides":
            kw, _ = shape(big=updating and cornell)
            steps.append(S("guides", spp=int(rng.integers(1, MAX_SPP + 1)), flags=_pick(rng, [0, TIME_KERNELS]), **kw))
        elif k == "sppm_create":
            kw, _ = shape(IMAGES[2:5])
            nm = "Z1" if "Z1" not in alive else "Z2"
            kw.update(name=nm, depth=4, light_depth=_pick(rng, LIGHT_DEPTHS), spl=_pick(rng, SPLS[1:]), radius=_pick(rng, RADII), alpha=_pick(rng, [0.5, 0.7]))
            alive[nm] = kw
            steps.append(S("sppm_create", **kw))
        elif k in ("sppm_render", "sppm_state", "sppm_reset", "sppm_destroy"):
            nm = _pick(rng, sorted(alive))
            if k == "sppm_render":
                steps.append(S(k, name=nm, passes=int(rng.integers(1, 3)), flags=_pick(rng, [0, COUNT_WORK])))
            else:
                steps.append(S(k, name=nm))
            if k == "sppm_destroy":
                del alive[nm]
        elif k in ("probe_closest", "probe_visibility"):
            steps.append(S(k, n=_pick(rng, [1, 257]), seed=int(rng.integers(0, 1 << 30))))
        elif k == "set_groups":
            steps.append(S(k, which=_pick(rng, ["file", "none"])))
        elif k == "refused":
            ok = [r[0] for r in REFUSALS if r[0] in R_REFUSALS] + (update_refusals(name) if updating else [])
            steps.append(refusal(_pick(rng, ok)))
        else:
            steps.append(S(k))
    return Session("R%d" % seed, name, "scene", steps)


def is_update_refusal(st):
    return st.kind == "refused" and st.kw["call"] in UPDATES


def update_conditions(session):
    """What the steps alone show about a session's updates, {condition: bool}: every accepted update hands over other
    records than the handle holds and is followed, before the next one, by a render that can show it; every refused update
    is followed by a PT, a BDPT and a PPM render and by an export of the tree."""
    steps, cur = session.steps, current(session.scene)
    changes = shown = rendered_on = True
    for i, st in enumerate(steps):
        if st.kind in UPDATES:
            nxt = next((j for j in range(i + 1, len(steps)) if steps[j].kind in UPDATES), len(steps))
            new = after_update(cur, st)
            changes &= new["edits"] != cur["edits"]
            shown &= any(p.kind in WITNESSES for p in steps[i + 1:nxt])
            cur = new
        elif is_update_refusal(st):
            rendered_on &= {"pt", "bdpt", "ppm", "export_bvh"} <= {p.kind for p in steps[i + 1:]}
    return dict(changes=changes, shown=shown, rendered_on=rendered_on)


def random_session(seed, first=0):
    """The session of a seed: the first attempt (first, first + 1, ...) that is not listed in R_REJECTED, meets every
    size condition and keeps the bidirectional table small; from R_UPDATING on also: holds two accepted updates and a
    refused one at least, every kind of render, and meets update_conditions().  A function of the seed alone."""
    attempt = first
    while True:
        s = _draw(seed, attempt)
        ok = attempt not in R_REJECTED[seed] and all(size_conditions(s).values()) and bdpt_table_bytes(s) <= BDPT_TABLE_LIMIT
        if ok and seed >= R_UPDATING:
            ok = (sum(st.kind in UPDATES for st in s.steps) >= 2 and any(is_update_refusal(st) for st in s.steps)
                  and all(update_conditions(s).values()) and set(WITNESSES) <= {st.kind for st in s.steps})
        if ok:
            return s, attempt
        attempt += 1


# ---- the table -------------------------------------------------------------------------------------------------------
_SESSIONS = {}


def session(name):
    if name not in _SESSIONS:
        make = dict(A=_session_a, A_fresh=_session_a_fresh, B=_session_b, C=_session_c, D=_session_d, E=_session_e, F=_session_f,
                    G=_session_g, G_rounds=_session_g_rounds, G_parallel=_session_g_parallel)
        _SESSIONS[name] = make[name]() if name in make else random_session(int(name[1:]))[0]
    return _SESSIONS[name]


UPDATING = ["G", "G_rounds", "G_parallel"] + ["R%d" % s for s in R_SEEDS if s >= R_UPDATING]       # the sessions with update steps
NAMES = ["A", "A_fresh", "B", "C", "D", "E", "F"] + ["R%d" % s for s in R_SEEDS[:R_UPDATING - 1]] + UPDATING
