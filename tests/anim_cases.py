"""Case table of the animation sessions: long, mixed sequences of the calls that change a live scene's triangles --
update_triangles, update_vertices_device, set_parts / pose, set_skin / skin, set_morphs / morph, rebuild, rebuild_device,
rebuild_device_bounded -- on ONE handle, with a host model of the whole handle state beside it.  The feature suites hold
each call to its definition and a few hand-picked pairs; these sessions hold every ordered pair, the kill-and-revive
chains, every order in which a scene comes to have both morphs and a deformer, a sixteen-frame animation and six seeded
random walks.  A plain module: no GPU, no tests.  tests/test_anim_cases_cpu.py holds the table to its conditions,
tests/test_gpu_anim_sessions.py runs it.

Scenes.  `bend`: skin_cases.data("bend"), twelve wall triangles and the 264-triangle sphere -- 828 corners across four
256-lane workgroups, two workgroups of the builder's kernels -- with its light and camera; `tiny3`: its first three
triangles; `none`: its rounds with zero triangles.  Every render is 32 x 24, depth 4, 2 spp.  `bend` has no sphere, so
the update_rounds step moves what its rounds do hold: the light and its light ball (same counts).

A session is Session(name, scene, steps), a step Step(kind, kw).  State-changing kinds: update_triangles,
update_vertices_device (kw edit), set_parts, pose (table), set_skin (skin), skin (table), set_morphs (morphs), morph (w),
rebuild, rebuild_device, rebuild_device_bounded (depth: "0", "need", "need+1", "19"), update_rounds (edit), keep_previous,
set_groups (which: "bend" / "none").  Observations: pt (walk: default, brute force, budget 1, budget 63, counting), bdpt,
ppm (null bounds), guides (with prev_position), probe_closest, probe_visibility, tree, records, infos.  `refused`: a call
that is illegal in the state the model is in at that step (kw label, call and the call's own arguments); code 1.

Arguments come from small pools by name (edit, rounds, parts, table, skin, morphs, depth resolve them for a scene): tables of two records built with
pose_cases.table / affine / rot_y / tilted -- identity, "turn:DEG", "twist:DEG", lift, nan1 (record 1 NaN: part or bone 1
dies; any finite table revives it), nan_all --; skins `height` (skin_cases.height_weights) and `onehot` (weights of 1.0f:
a pose, byte for byte); target sets `four` (a radial bulge, an EMPTY target, a target of NaN deltas, a lift of every
corner) and `two` (morph_cases.two_shapes); weights given literally, among them all zeros, -0.0, a negative weight, a
weight on the empty target, the NaN target under weight 0 and under 1, and (session K) an infinite one.

The model.  Model restates include/hpt.h ("scene updates", "poses", "skinning", "morph targets", "motion", "rebuild",
"device builds", "bounded device builds") in numpy plus the library's host definitions, and nothing of the library's
update code: L, sp; the rest pose R; targets and weights; one deformer (parts or a skin) and its table (None: identity
since the last capture); cur; prev (G'); motion; the update counts; tree = (kind, depth, L, sp, T at build time); the
counters of rebuild_info, device_build_info and bounded_build_info.  set_parts, set_skin, set_morphs and the two updates
capture (R = cur, weights zero, table None); M = morph_host(R, weights), cur = deformer(table)(M).  A build changes the
tree and the counters only.  A refused call changes nothing.  The expected tree after any step is the definition of
tree.kind built from T and refitted to cur: refit_bvh_host (created, host), device_build_bvh_host (device),
device_build_bounded_bvh_host (bounded) -- one rule: the CPU suite asserts that the host builder's export of every T the
sessions build from equals its refit to T.  Mutant models (Model(mutant=...)): (i) the deformer applied to R instead of
M; (ii) weights not zeroed at a capture; (iii) the table kept across a capture; (iv) set_parts / set_skin not dropping
each other's deformer; (v) a morph on a deformed scene skipping the deformer; (vi) the tree refitted from the creation
topology after a build; (vii) a build's T taken as the rest pose; (viii) keep_previous ignored.

Sessions.  P "every pair": a greedy walk over the eleven triangle-state kinds until all 121 ordered pairs have occurred as
consecutive steps; where b is illegal after a the step is b's refused form and the walk goes on from a's state; records,
tree and a pt whose walk cycles follow every step.  K "killed and revived": a NaN part table, the three builds while the
part is dead, a table of NaNs alone (every triangle dead) and the three builds again, a finite pose; the same with a
skin's NaN bone and an infinite morph weight.  M1..M4 "M's first allocation": morphs (at non-zero weights) then parts,
morphs then a skin, parts (posed) then morphs, a skin (skinned) then morphs -- one handle each, as the buffer is allocated
once per handle --, a morph directly, one after a table, the deformer swapped twice with a morph between.  F "frames":
sixteen frames of keep_previous, morph, skin (pose from frame 8), guides, pt; a build of another kind every fourth frame;
update_rounds, set_groups and bdpt in the middle.  T: P's first forty steps on tiny3.  Z: every call once on none.
A1..A6: 40 steps each from numpy.random.default_rng(seed) over the whole vocabulary, refusals included, legality decided
by the model.

Observed numbers (tests/test_anim_cases_cpu.py prints them, and asserts the step counts, the pairs, the bounds and the mutant
table):
%(NUMBERS)s
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

import bounded_oracle as bo                                        # noqa: E402
import device_build_cases as dc                                    # noqa: E402
import morph_cases as mc                                           # noqa: E402
import motion_oracle                                              # noqa: E402
import pose_cases as pc                                            # noqa: E402
import pose_oracle as po                                           # noqa: E402
import ppm_oracle                                                  # noqa: E402
import refit_cases as rc                                           # noqa: E402
import session_cases as ssc                                        # noqa: E402
import skin_cases as sc                                            # noqa: E402
from path_tracing_amd import scene_io as sio                       # noqa: E402

NUMBERS = """  P     540 steps, 135 of them state-changing or refused; 121 of 121 ordered pairs; 4 pairs are refusals, the ones no
        state makes legal: (set_parts, skin), (pose, skin), (set_skin, pose), (skin, pose)
  T     40 steps on three triangles; Z 26 steps on none; K 207, M1 .. M4 98 each, F 96, A1 .. A6 40 each
  byte-equal accepted geometry steps (update_*, pose, skin, morph) of all such steps, every one of them an identity table or
  all-zero weights: P 22 / 58, K 0 / 8, M1 .. M4 0 / 10, F 0 / 32, T 1 / 8, A1 1 / 9 (0.11), A2 3 / 10 (0.30), A3 2 / 8 (0.25),
  A4 1 / 11 (0.09), A5 3 / 12 (0.25), A6 1 / 10 (0.10); the bound is one half
  lit pixels of the dimmest pt / bdpt / ppm oracle image outside K's all-dead steps and Z: P 0.67, K 0.50, M1 M2 0.63, M3 M4 0.82,
  F 0.78, T 0.67, A1 0.55, A2 0.80, A3 0.81, A4 .. A6 0.82; the bound is one half
  trees: bvh_depth 0 .. 15, never above 30 and never above a bounded build's max_depth; 34 bounded builds, forced_nodes 0 .. 116,
  both 0 and > 0 occur; the host builder's export equals its refit on each of the 33 record sets a created or host tree is of
  mutants, the first (session, step, what) among P, M1 .. M4, F that tells each apart, and the random sessions that do:
    i    P 288 cur     A1 A2 A3 A4 A5 A6        v     M1 20 cur     A4 A6
    ii   P 324 cur     A1 A2 A4 A6              vi    P 64 tree     A1 A2 A3 A4 A5 A6
    iii  P 56 cur      A1 A2 A3                 vii   F 22 tree     A1 A2 A3 A4 A5
    iv   P 232 cur     A1 A2 A3 A5              viii  F 10 guide    A3 A5
  seeds: A1 .. A6 are default_rng(1, 2, 3, 9, 23, 6).  Seeds 4 and 5 were replaced by 9 and 23: with 1 .. 6 only one session
  told mutant v apart (seed 6) and only one mutant viii (seed 3)
  the GPU half on an MI355X: %(TIMES)s"""
TIMES = "P 0.40 s, K 0.17 s, F 0.13 s, M1 .. M4 0.06 s each, T, Z and A1 .. A6 under 0.05 s each, the twins 0.51 s; 19 tests, 1.7 s in all"
NUMBERS = NUMBERS % dict(TIMES=TIMES)
__doc__ = __doc__ % dict(NUMBERS=NUMBERS)

F32, U32 = np.float32, np.uint32
W, H, DEPTH, SPP, SEED = dc.W, dc.H, dc.DEPTH, dc.SPP, dc.SEED
NWALL = rc.NWALL
INF, NAN = float("inf"), float("nan")
ERR_INVALID = 1
N_PROBE = 257
BDPT = dict(eye_depth=4, light_depth=4, spp=SPP, spl=8, seed=3)
PPM = dict(eye_depth=4, light_depth=4, spp=1, spl=1024, radius=0.1, seed=5)
GUIDE_SEED = 7

Step = collections.namedtuple("Step", "kind kw")
Session = collections.namedtuple("Session", "name scene steps")

TRI_KINDS = ("update_triangles", "update_vertices_device", "set_parts", "pose", "set_skin", "skin", "set_morphs", "morph",
             "rebuild", "rebuild_device", "rebuild_device_bounded")
STATE_KINDS = TRI_KINDS + ("update_rounds", "keep_previous", "set_groups")
GEOMETRY_KINDS = ("update_triangles", "update_vertices_device", "pose", "skin", "morph")      # the triangle updates
BUILD_KINDS = ("rebuild", "rebuild_device", "rebuild_device_bounded")
OBSERVATIONS = ("pt", "bdpt", "ppm", "guides", "probe_closest", "probe_visibility", "tree", "records", "infos")
WALKS = ("default", "brute force", "budget 1", "budget 63", "counting")
DEPTHS = ("0", "need", "need+1", "19")
MUTANTS = ("i", "ii", "iii", "iv", "v", "vi", "vii", "viii")

EDITS = ("base", "wide", "low", "moved")
TABLES = ("identity", "turn:30", "turn:75", "twist:20", "twist:90", "lift", "nan1")
SKINS = ("height", "onehot")
MORPHS = ("four", "two")
NEG0 = -0.0
WEIGHTS = {4: ((0.0, 0.0, 0.0, 0.0), (NEG0, 0.0, NEG0, 0.0), (0.8, 3.0, 0.0, 0.0), (0.2, 0.0, NEG0, 1.0), (-0.45, 0.0, 0.0, 0.5),
               (0.5, 0.0, 1.0, 0.0)),
           2: ((0.0, NEG0), (0.8, 0.0), (0.2, 1.0), (-0.3, 0.6))}
ROUNDS = ("base", "moved")
GROUPS = ("bend", "none")

# label -> (call, the kinds of state in which the label is what refuses the call)
REFUSALS = collections.OrderedDict([
    ("pose, no parts", "pose"), ("skin, no skin", "skin"), ("morph, no morphs", "morph"),
    ("pose, wrong record count", "pose"), ("skin, wrong bone count", "skin"), ("morph, wrong target count", "morph"),
    ("set_skin, a bone out of range", "set_skin"), ("set_skin, a negative weight", "set_skin"),
    ("set_morphs, corners not ascending", "set_morphs"),
    ("bounded, below need", "rebuild_device_bounded"), ("bounded, 31", "rebuild_device_bounded"), ("bounded, negative", "rebuild_device_bounded"),
    ("update_triangles, a short array", "update_triangles"),
])


def S(kind, **kw):
    return Step(kind, kw)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene(name):
    """dict(name, L, sp, tr, n, first, centre, order, default_order, need) of a session's scene, once per process."""
    if name not in _SCENES:
        d = sc.data("bend")
        tr = dict(bend=d.tr, tiny3=d.tr[:3].copy(), none=d.tr[:0].copy())[name]
        first = NWALL if len(tr) > NWALL else 0
        v = po.verts_of(tr)[first:].reshape(-1, 3).astype(np.float64)
        centre = v.mean(axis=0) if len(v) else np.zeros(3)
        for a in (d.L, d.sp, tr):
            a.setflags(write=False)
        _SCENES[name] = dict(name=name, L=d.L, sp=d.sp, tr=tr, n=len(tr), first=first, centre=centre, order=rc._order(d.sp, tr),
                             default_order=sio.object_order(None, d.sp, tr), need=bo.need(len(tr)), eye=d.eye, look=d.look)
        if name == "tiny3":                                          # two floor triangles and one of a wall, seen from above: lit on 2 / 3 of the image
            _SCENES[name].update(eye=(0.0, 0.4, -0.3), look=(0.0, -0.5, 0.0))
    return _SCENES[name]


def camera(sd):
    return sio.make_camera(sd["eye"], sd["look"], sio.CORNELL_UP, 50.0, W, H)


def bdpt_camera(sd):
    return sio.make_camera(sd["eye"], sd["look"], sio.CORNELL_UP, 50.0, W, H, tan_in_float=True)


# ---- the pools -------------------------------------------------------------------------------------------------------------
def edit(sd, name):
    """The records of a triangle edit: a pure function of the scene's base records."""
    tr, first = sd["tr"], sd["first"]
    if name == "base" or not len(tr):
        return tr
    v = po.verts_of(tr).astype(np.float64)
    if name == "wide":
        v[first:] = (v[first:] - sd["centre"]) * 1.4 + sd["centre"]
    elif name == "low":
        v[first:, :, 1] -= 0.08
    elif name == "moved":
        v[first:] += np.random.default_rng(3).uniform(-0.05, 0.05, (len(tr) - first, 1, 3))
    else:
        raise KeyError(name)
    return po.with_verts(tr, v.astype(F32))


def rounds(sd, name):
    L = sd["L"]
    if name == "moved":
        L = L.copy()
        pos = np.array((0.2, 0.35, 0.3), F32)
        L[0]["pos"] = pos
        L[0]["light_ball"]["center"] = pos
    return L, sd["sp"]


def parts(sd):
    n = sd["n"]
    return (pc.two_parts(n) if n > NWALL else (np.arange(n, dtype=np.int32) % 2).astype(np.int32)), 2


def table(sd, name, records=2):
    c = sd["centre"]
    nan_rec = np.full((3, 4), NAN, F32)
    if name == "identity":
        t = pc.identity(2)
    elif name.startswith("turn:"):
        t = pc.table(po.IDENTITY, pc.affine(pc.tilted(float(name[5:])), c))
    elif name.startswith("twist:"):
        t = pc.table(po.IDENTITY, pc.affine(pc.rot_y(float(name[6:])), c))
    elif name == "lift":
        t = pc.table(pc.affine(np.eye(3), shift=(0.0, 0.0, 0.0)), pc.affine(np.eye(3) * 0.8, c, (0.05, 0.1, -0.05)))
    elif name == "nan1":
        t = pc.table(po.IDENTITY, nan_rec)
    elif name == "nan_all":
        t = pc.table(nan_rec, nan_rec)
    else:
        raise KeyError(name)
    return t if records == 2 else np.concatenate([t, pc.identity(records - 2)])


def skin(sd, name):
    """(corner_bone, corner_weight, num_bones)."""
    tr, n = sd["tr"], sd["n"]
    if name == "height":
        bone, weight = sc.height_weights(tr, first=sd["first"]) if n else sc.no_weights(0)
    elif name == "onehot":
        bone, weight = sc.no_weights(n)
        bone[:, :, 0] = parts(sd)[0][:, None]
        weight[:, :, 0] = F32(1)
    else:
        raise KeyError(name)
    return bone, weight, 2


def morphs(sd, name):
    """(target_begin, entry_corner, entry_delta)."""
    tr, n, first, c = sd["tr"], sd["n"], sd["first"], sd["centre"]
    if not n:
        return mc.targets(*([mc.EMPTY] * (4 if name == "four" else 2)))
    if name == "four":
        a, b = first + (n - first) // 3, first + (n - first) // 2 + 1
        nan_d = mc.const(a, b, (NAN, 0.0, INF))
        if first:                                                   # ... and the first corners of two walls
            nan_d = (np.concatenate([mc.corners_of(0, 2), nan_d[0]]), np.concatenate([np.full((6, 3), NAN, F32), nan_d[1]]))
        every = mc.corners_of(0, n), np.tile(np.array((0.0, 0.04, 0.0), F32), (3 * n, 1))
        return mc.targets(mc.radial(tr, first, n, c, 0.5), mc.EMPTY, nan_d, every)
    if name == "two":
        return mc.two_shapes(tr, first=first, centre=c)
    raise KeyError(name)


def depth(sd, name):
    return dict([("0", 0), ("need", sd["need"]), ("need+1", sd["need"] + 1), ("19", 19)])[name]


def weights(w):
    return np.array(w, F32)


def all_inactive(w):
    return not ((weights(w).view(U32) << np.uint32(1)) != 0).any()


def refused_args(sd, model, kw):
    """(method name, arguments) of a refused step's call: the valid call with the one thing wrong that the label names."""
    label = kw["label"]
    if label in ("pose, no parts", "skin, no skin"):
        return kw["call"], (table(sd, kw["table"]),)
    if label == "morph, no morphs":
        return "morph", (weights(kw["w"]),)
    if label in ("pose, wrong record count", "skin, wrong bone count"):
        return kw["call"], (table(sd, "turn:30", records=3),)
    if label == "morph, wrong target count":
        return "morph", (np.full(len(model.targets[0]), 0.5, F32),)                  # one weight too many
    if label.startswith("set_skin"):
        bone, weight, nb = skin(sd, "height")
        bone, weight = bone.copy(), weight.copy()
        at = sd["n"] // 2
        if "bone" in label:
            bone[at, 1, 3] = nb                                      # an inactive influence: refused all the same
        else:
            weight[at, 2, 1] = F32(-0.25)
        return "set_skin", (bone, weight, nb)
    if label.startswith("set_morphs"):
        tb, ec, ed = morphs(sd, "two")
        ec = ec.copy()
        ec[[3, 4]] = ec[[4, 3]]
        return "set_morphs", (tb, ec, ed)
    if label.startswith("bounded"):
        return "rebuild_device_bounded", (dict([("bounded, below need", sd["need"] - 1), ("bounded, 31", 31), ("bounded, negative", -2)])[label],)
    if label.startswith("update_triangles"):
        return "update_triangles", (model.cur[:-1],)
    raise KeyError(label)


def available(sd, model, label):
    """Whether the label names what refuses the call in the model's state on this scene."""
    has = dict(parts=model.deformer is not None and model.deformer[0] == "parts", skin=model.deformer is not None and model.deformer[0] == "skin",
               morphs=model.targets is not None)
    if label == "pose, no parts":
        return not has["parts"]
    if label == "skin, no skin":
        return not has["skin"]
    if label == "morph, no morphs":
        return not has["morphs"]
    if label == "pose, wrong record count":
        return has["parts"]
    if label == "skin, wrong bone count":
        return has["skin"]
    if label == "morph, wrong target count":
        return has["morphs"]
    if label == "bounded, below need":
        return sd["need"] > 1                                         # (need - 1 = 0 would mean 30)
    if label.startswith("set_skin") or label.startswith("update_triangles"):
        return sd["n"] > 0
    if label.startswith("set_morphs"):
        return sd["n"] > 1
    return True


# ---- the model -------------------------------------------------------------------------------------------------------------
Tree = collections.namedtuple("Tree", "kind depth L sp T")
Snap = collections.namedtuple("Snap", "cur L sp prev_tr prev_sp motion updates live dead tree rebuilds builds fell_back bounded order accepted "
                                      "R targets weights deformer table")
ZERO_BOUNDED = dict(max_depth=0, forced_nodes=0, first_forced_level=0)


class Model:
    """The handle's state by include/hpt.h.  `hpt` gives the host definitions (no device).  mutant: one of MUTANTS."""

    def __init__(self, hpt, sd, mutant=None):
        self.hpt, self.sd, self.mutant = hpt, sd, mutant
        self.L, self.sp = sd["L"], sd["sp"]
        self.cur = self.R = sd["tr"]
        self.targets = self.weights = self.deformer = self.table = None
        self.stale = None                                            # mutant iv: the deformer that should have been dropped
        self.prev = (sd["tr"], sd["sp"])
        self.motion = False
        self.updates = self.live = self.dead = 0
        self.tree = Tree("created", 0, self.L, self.sp, sd["tr"])
        self.rebuilds = self.builds = self.fell_back = 0
        self.bounded = dict(ZERO_BOUNDED)
        self.order = sd["default_order"]
        self.accepted = True                                         # whether the last step's call was accepted

    # -- the definitions ----------------------------------------------------------------------------------------------
    def morphed(self):
        if self.targets is None:
            return self.R
        return self.hpt.morph_host(self.R, *self.targets, self.weights)

    def deformed(self, m, deformer=None):
        deformer = deformer or self.deformer
        if deformer is None or self.table is None:
            return m
        if deformer[0] == "parts":
            return self.hpt.pose_host(m, deformer[1], self.table)
        return self.hpt.skin_host(m, deformer[1], deformer[2], self.table)

    def compose(self):
        return self.deformed(self.R if self.mutant == "i" else self.morphed())

    def refusal(self, kind, kw):
        """The label under which the call is refused in this state, or None."""
        d = self.deformer
        if kind == "pose" and (d is None or d[0] != "parts"):
            return "pose, no parts"
        if kind == "skin" and (d is None or d[0] != "skin"):
            return "skin, no skin"
        if kind == "morph":
            if self.targets is None:
                return "morph, no morphs"
            if len(kw["w"]) != len(self.targets[0]) - 1:
                return "morph, wrong target count"
        if kind == "rebuild_device_bounded":
            D = depth(self.sd, kw["depth"])
            if bo.effective_depth(self.sd["n"], D) is None:
                return "bounded, negative" if D < 0 else "bounded, 31" if D > bo.MAX_BVH_DEPTH else "bounded, below need"
        return None

    # -- the transitions ----------------------------------------------------------------------------------------------
    def _capture(self):
        self.R = self.cur
        if self.targets is not None and self.mutant != "ii":
            self.weights = np.zeros(len(self.targets[0]) - 1, F32)
        if self.mutant != "iii":
            self.table = None

    def _updated(self):
        d = int(rc.dead(self.cur).sum())
        self.updates, self.live, self.dead, self.motion = self.updates + 1, len(self.cur) - d, d, True

    def _build_from(self):
        return self.R if self.mutant == "vii" else self.cur

    def apply(self, st):
        sd, k, kw = self.sd, st.kind, st.kw
        self.accepted = k != "refused"
        if k == "refused":
            # mutant iv still holds the other deformer, and takes the call
            if self.mutant == "iv" and self.stale is not None and kw["label"] == ("pose, no parts" if self.stale[0] == "parts" else "skin, no skin"):
                self.table = table(sd, kw["table"])
                self.cur = self.deformed(self.R if self.mutant == "i" else self.morphed(), self.stale)
                self._updated()
            return
        if k in ("update_triangles", "update_vertices_device"):
            self.cur = edit(sd, kw["edit"])
            self._capture()
            self._updated()
        elif k == "set_parts":
            self.stale, self.deformer = self.deformer if self.deformer and self.deformer[0] == "skin" else self.stale, ("parts", parts(sd)[0])
            self._capture()
        elif k == "set_skin":
            self.stale, self.deformer = self.deformer if self.deformer and self.deformer[0] == "parts" else self.stale, ("skin",) + skin(sd, kw["skin"])[:2]
            self._capture()
        elif k == "set_morphs":
            self.targets = morphs(sd, kw["morphs"])
            self.weights = np.zeros(len(self.targets[0]) - 1, F32)
            self._capture()
        elif k in ("pose", "skin"):
            self.table = table(sd, kw["table"])
            self.cur = self.compose()
            self._updated()
        elif k == "morph":
            self.weights = weights(kw["w"])
            self.cur = self.morphed() if self.mutant == "v" else self.compose()
            self._updated()
        elif k == "rebuild":
            self.rebuilds += 1
            if self.mutant != "vi":
                self.tree = Tree("host", 0, self.L, self.sp, self._build_from())
        elif k in ("rebuild_device", "rebuild_device_bounded"):
            T = self._build_from()
            D = depth(sd, kw["depth"]) if k == "rebuild_device_bounded" else 0
            want = (self.hpt.device_build_bounded_bvh_host(self.L, self.sp, T, None, D) if k == "rebuild_device_bounded"
                    else self.hpt.device_build_bvh_host(self.L, self.sp, T))
            self.builds += 1
            self.fell_back = int(want["build"]["fell_back"])
            self.rebuilds += self.fell_back
            if k == "rebuild_device_bounded":
                self.bounded = dict(want["bounded"])
            if self.mutant != "vi":
                kind = "host" if self.fell_back else ("bounded" if k == "rebuild_device_bounded" else "device")
                self.tree = Tree(kind, D, self.L, self.sp, T)
        elif k == "update_rounds":
            self.L, self.sp = rounds(sd, kw["edit"])
            self.motion = True
        elif k == "keep_previous":
            if self.mutant != "viii":
                self.prev, self.motion = (self.cur, self.sp), False
        elif k == "set_groups":
            self.order = sd["order"] if kw["which"] == "bend" else sd["default_order"]
        elif k not in OBSERVATIONS:
            raise ValueError(k)

    def snap(self):
        return Snap(self.cur, self.L, self.sp, self.prev[0], self.prev[1], self.motion, self.updates, self.live, self.dead, self.tree,
                    self.rebuilds, self.builds, self.fell_back, dict(self.bounded), self.order, self.accepted,
                    self.R, self.targets, self.weights, self.deformer, self.table)


def replay(hpt, session, mutant=None):
    """One Snap per step: the model's state after it."""
    m = Model(hpt, scene(session.scene), mutant)
    out = []
    for st in session.steps:
        m.apply(st)
        out.append(m.snap())
    return out


_TREES = {}


def expected_tree(hpt, tree, cur):
    """The definition of tree.kind built from the tree's T and refitted to cur, once per process."""
    key = (tree.kind, tree.depth, tree.L.tobytes(), tree.T.tobytes(), cur.tobytes())
    if key not in _TREES:
        if tree.kind in ("created", "host"):
            _TREES[key] = hpt.refit_bvh_host(tree.L, tree.sp, tree.T, cur)
        elif tree.kind == "device":
            _TREES[key] = hpt.device_build_bvh_host(tree.L, tree.sp, tree.T, cur)
        else:
            _TREES[key] = hpt.device_build_bounded_bvh_host(tree.L, tree.sp, tree.T, cur, tree.depth)
    return _TREES[key]


def tree_bytes(t):
    return b"".join(np.ascontiguousarray(t[k]).tobytes() for k in ("num_nodes", "num_tris", "bvh_depth", "qorigin", "qscale", "qnodes", "tris"))


# ---- expected images and probes --------------------------------------------------------------------------------------------
class Oracles:
    """`pt` the oracle package (PT, BDPT, the scans), the photon-mapping and motion-guide libraries built into out_dir."""

    def __init__(self, oracle_mod, out_dir):
        self.pt = oracle_mod
        self.ppm = ppm_oracle.build(out_dir)
        self.motion = motion_oracle.build(out_dir)


_IMAGES = {}


def _once(key, make):
    if key not in _IMAGES:
        e = make()
        for v in (e.values() if isinstance(e, dict) else e if isinstance(e, tuple) else [e]):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _IMAGES[key] = e
    return _IMAGES[key]


def pt_image(orc, sd, snap):
    """(image, stats) of the oracle's scan of the snapshot's records: the seed is fixed, so two snapshots of the same
    bytes share one image and a changed image means changed geometry."""
    return _once(("pt", sd["name"], snap.L.tobytes(), snap.cur.tobytes()),
                 lambda: orc.pt.pt_render(snap.L, snap.sp, snap.cur, camera(sd), W, H, DEPTH, SPP, seed=SEED))


def live_bounds(sp, tr):
    """ppm_oracle.scene_bounds of the spheres and the live triangles; the unit cube where there is nothing."""
    live = tr[~rc.dead(tr)]
    if not len(live) and not len(sp):
        return np.zeros(3, F32), np.ones(3, F32)
    return ppm_oracle.scene_bounds(sp, live)


def probe_rays(snap, seed):
    lo, hi = live_bounds(snap.sp, snap.cur)
    return ssc.probe_rays(dict(lo=lo, hi=hi), N_PROBE, seed)


def observe(orc, sd, snap, st):
    """The expected result of the observation step `st` on the snapshot: a dict of arrays (pt: also `stats`)."""
    k, kw = st.kind, st.kw
    if k == "pt":
        img, stats = pt_image(orc, sd, snap)
        return dict(image=img, stats=stats)
    if k == "bdpt":
        kind, index, group = snap.order
        key = ("bdpt", sd["name"], snap.L.tobytes(), snap.cur.tobytes(), np.asarray(group).tobytes())
        return dict(image=_once(key, lambda: orc.pt.bdpt_render(snap.L, snap.sp, snap.cur, snap.order, sd["eye"], sd["look"], sio.CORNELL_UP, 50.0, W, H,
                                                                 BDPT["eye_depth"], BDPT["light_depth"], BDPT["spp"], BDPT["spl"], seed=BDPT["seed"])[0]))
    if k == "ppm":
        lo, hi = ppm_oracle.scene_bounds(snap.sp, snap.cur[~rc.dead(snap.cur)])
        key = ("ppm", sd["name"], snap.L.tobytes(), snap.cur.tobytes())
        return dict(image=_once(key, lambda: ppm_oracle.render(orc.ppm, snap.L, snap.sp, snap.cur, camera(sd), W, H, PPM["eye_depth"], PPM["light_depth"],
                                                                PPM["spp"], PPM["spl"], PPM["radius"], seed=PPM["seed"], scene_min=lo, scene_max=hi)[0]))
    if k == "guides":
        key = ("guides", sd["name"], snap.L.tobytes(), snap.cur.tobytes(), snap.prev_tr.tobytes(), snap.prev_sp.tobytes())
        return _once(key, lambda: motion_oracle.render(orc.motion, snap.L, snap.sp, snap.cur, snap.prev_sp, snap.prev_tr, camera(sd), W, H, SPP, seed=GUIDE_SEED)[0])
    if k == "probe_closest":
        o, d, _ = probe_rays(snap, kw["seed"])
        t, prim = orc.pt.closest_hits(snap.L, snap.sp, snap.cur, o, d)
        return dict(t=t, prim=prim)
    if k == "probe_visibility":
        o, _, p2 = probe_rays(snap, kw["seed"])
        return dict(visible=orc.pt.visibility(snap.sp, snap.cur, o, p2))
    return None


# ---- building sessions -----------------------------------------------------------------------------------------------------
class Builder:
    """Appends steps to a session, the model beside it deciding what is legal: an illegal call becomes its refused form."""

    def __init__(self, hpt, name, scene_name):
        self.hpt, self.name, self.sd = hpt, name, scene(scene_name)
        self.model, self.steps, self.walk = Model(hpt, self.sd), [], 0

    def add(self, kind, **kw):
        """The step, or its refused form; returns True where the call is accepted."""
        label = self.model.refusal(kind, kw) if kind in STATE_KINDS else None
        st = S(kind, **kw) if label is None else S("refused", label=label, call=kind, **kw)
        self.steps.append(st)
        self.model.apply(st)
        return label is None

    def refuse(self, label, **kw):
        """The refused step `label`, where this state and scene have it; the arguments the labels of a missing deformer need
        are given by the caller."""
        if not available(self.sd, self.model, label):
            return False
        call = REFUSALS[label]
        if label in ("pose, no parts", "skin, no skin"):
            kw.setdefault("table", "turn:30")
        if label == "morph, no morphs":
            kw.setdefault("w", WEIGHTS[4][2])
        self.steps.append(S("refused", label=label, call=call, **kw))
        self.model.apply(self.steps[-1])
        return True

    def pt(self):
        self.add("pt", walk=WALKS[self.walk % len(WALKS)])
        self.walk += 1

    def watch(self):
        self.add("records")
        self.add("tree")
        self.pt()

    def visible(self, kind, kw):
        """Whether the accepted step would change cur's bytes, or is one that is expected not to."""
        if kind not in GEOMETRY_KINDS or self.model.refusal(kind, kw) is not None:
            return True
        trial = Model(self.hpt, self.sd)
        trial.__dict__.update({k: v for k, v in self.model.__dict__.items()})
        trial.bounded = dict(self.model.bounded)
        trial.apply(S(kind, **kw))
        a, b = self.model.cur, trial.cur
        if a.tobytes() == b.tobytes():
            return (kind in ("pose", "skin") and kw["table"] == "identity") or (kind == "morph" and all_inactive(kw["w"]))
        # ... in a triangle that is live before or after: corners that move inside a dead triangle reach no pixel
        changed = (po.verts_of(a).view(U32) != po.verts_of(b).view(U32)).reshape(len(a), -1).any(axis=1)
        return bool((changed & ~(rc.dead(a) & rc.dead(b))).any())

    def choose(self, kind, pick):
        """Arguments of a step of `kind` from the pools; pick(pool) chooses.  Redrawn (up to eight times) while the step would
        leave the geometry's bytes alone without being an identity table or all-zero weights."""
        m = self.model
        for _ in range(8):
            if kind in ("update_triangles", "update_vertices_device"):
                kw = dict(edit=pick(EDITS))
            elif kind in ("pose", "skin"):
                kw = dict(table=pick(TABLES))
            elif kind == "set_skin":
                kw = dict(skin=pick(SKINS))
            elif kind == "set_morphs":
                kw = dict(morphs=pick(MORPHS))
            elif kind == "morph":
                kw = dict(w=pick(WEIGHTS[len(m.targets[0]) - 1 if m.targets is not None else 4]))
            elif kind == "rebuild_device_bounded":
                kw = dict(depth=pick(DEPTHS))
            elif kind == "update_rounds":
                kw = dict(edit=pick(ROUNDS))
            elif kind == "set_groups":
                kw = dict(which=pick(GROUPS))
            elif kind in ("probe_closest", "probe_visibility"):
                kw = dict(seed=100 + len(self.steps))
            elif kind == "pt":
                kw = dict(walk=pick(WALKS))
            else:
                kw = {}
            if self.visible(kind, kw):
                return kw
        return None

    def session(self):
        return Session(self.name, self.sd["name"], self.steps)


class _Cycle:
    """pick(pool): the pool's entries in turn, one counter per pool."""

    def __init__(self):
        self.at = collections.Counter()

    def __call__(self, pool):
        self.at[pool] += 1
        return pool[(self.at[pool] - 1) % len(pool)]


_ENABLES = dict(pose="set_parts", skin="set_skin", morph="set_morphs")
# one deformer per scene: after these a, b finds the other deformer whatever came before
ALWAYS_REFUSED = {("set_parts", "skin"), ("pose", "skin"), ("set_skin", "pose"), ("skin", "pose")}


def _legal(model, kind):
    """Whether a call of `kind` with arguments from the pools is accepted in the model's state."""
    if kind == "pose":
        return model.deformer is not None and model.deformer[0] == "parts"
    if kind == "skin":
        return model.deformer is not None and model.deformer[0] == "skin"
    if kind == "morph":
        return model.targets is not None
    return True                                                      # the set_ calls, the updates and the builds at the pools' depths


def _session_p(hpt):
    b, pick = Builder(hpt, "P", "bend"), _Cycle()
    todo = {(x, y) for x in TRI_KINDS for y in TRI_KINDS}
    left = lambda c: sum((c, z) in todo for z in TRI_KINDS)
    last = None
    while todo:
        nxt = [y for y in TRI_KINDS if (last, y) in todo]
        if nxt:
            # a legal one first; then one that no state makes legal after `last`, as its refusal; one that only this state
            # makes illegal waits for the set_ call that cures it, and the walk comes back to the pair
            y = ([y for y in nxt if _legal(b.model, y)] or [y for y in nxt if (last, y) in ALWAYS_REFUSED] or [_ENABLES[nxt[0]]])[0]
        else:                                                        # every pair from `last` has occurred: go where the most are left
            legal = [c for c in TRI_KINDS if left(c) and _legal(b.model, c)]
            y = max(legal, key=left) if legal else _ENABLES[[c for c in TRI_KINDS if left(c)][0]]
        kw = b.choose(y, pick)
        if kw is None:                                               # nothing in the pool would show: fresh records first
            y = "update_triangles"
            kw = b.choose(y, pick)
        ok = b.add(y, **kw)
        todo.discard((last, y))
        b.watch()
        if ok:
            last = y
    return b.session()


def _builds(b, pt=True):
    for kind, kw in (("rebuild", {}), ("rebuild_device", {}), ("rebuild_device_bounded", dict(depth="need+1"))):
        b.add(kind, **kw)
        b.watch() if pt else (b.add("records"), b.add("tree"))


def _refusals(b):
    """Every refusal this state and scene have, the handle checked after each."""
    for label in REFUSALS:
        if b.refuse(label):
            b.watch()


def _session_k(hpt):
    b = Builder(hpt, "K", "bend")
    _refusals(b)                                                     # nothing set: every call that misses its set_ call
    b.add("set_groups", which="bend")

    def others():
        b.add("bdpt"); b.add("ppm"); b.add("guides"); b.add("probe_closest", seed=11); b.add("probe_visibility", seed=12); b.add("infos")
    b.add("set_parts")
    b.add("pose", table="nan1"); b.watch(); others()
    _builds(b)
    b.add("pose", table="nan_all"); b.watch(); b.add("probe_closest", seed=13); b.add("infos")        # every triangle dead
    _builds(b)
    b.add("pose", table="turn:30"); b.watch(); others()
    b.add("set_skin", skin="height")
    b.add("skin", table="nan1"); b.watch(); others()
    _builds(b)
    b.add("keep_previous")
    b.add("skin", table="twist:20"); b.watch(); others()
    b.add("set_morphs", morphs="four")
    b.add("morph", w=(0.5, 0.0, 1.0, 0.0)); b.watch(); others()                                       # the NaN target: 48 triangles dead
    b.add("morph", w=(0.0, 0.0, 0.0, INF)); b.watch(); b.add("probe_visibility", seed=14); b.add("infos")      # every triangle dead
    _builds(b)
    b.add("morph", w=(0.8, 3.0, 0.0, 0.0)); b.watch(); others()
    _refusals(b)                                                     # a skin and morphs: the wrong counts, the arrays with one thing wrong
    b.add("set_groups", which="none")
    b.add("bdpt")
    return b.session()


def _session_m(hpt, which):
    b = Builder(hpt, "M%d" % which, "bend")
    wa, wb, wc = WEIGHTS[4][2], WEIGHTS[4][3], WEIGHTS[4][4]
    first, second = (("set_parts", {}, "pose"), ("set_skin", dict(skin="height"), "skin"))[::1 if which in (1, 3) else -1]
    if which in (1, 2):                                              # morphs first, at non-zero weights, then the deformer
        b.add("set_morphs", morphs="four"); b.watch()
        b.add("morph", w=wa); b.watch()
        b.add(first[0], **first[1]); b.watch()
    else:                                                            # the deformer first, under a table, then morphs
        b.add(first[0], **first[1]); b.watch()
        b.add(first[2], table="turn:30"); b.watch()
        b.add("set_morphs", morphs="four"); b.watch()
    b.add("morph", w=wb); b.watch()                                  # directly: the deformer is still at identity
    b.add(first[2], table="twist:90"); b.watch()
    b.add("morph", w=wc); b.watch()
    b.add("guides")
    for dfm in (second, first):                                      # swapped twice, a morph between
        b.add(dfm[0], **dfm[1]); b.watch()
        b.add("morph", w=wa); b.watch()
        b.add(dfm[2], table="turn:75"); b.watch()
        b.add("morph", w=wb); b.watch()
    _refusals(b)
    b.add("infos")
    return b.session()


def _session_f(hpt):
    b = Builder(hpt, "F", "bend")
    b.add("set_skin", skin="height")
    b.add("set_morphs", morphs="four")
    builds = (("rebuild", {}), ("rebuild_device", {}), ("rebuild_device_bounded", dict(depth="need")), ("rebuild_device_bounded", dict(depth="19")))
    for f in range(16):
        if f == 8:
            b.add("update_rounds", edit="moved")
            b.add("set_groups", which="bend")
            b.add("bdpt")
            b.add("set_parts")
        b.add("keep_previous")
        b.add("morph", w=(0.05 * (f + 1), 0.0, 0.0, 0.1 * (f % 5) - 0.2))
        b.add("skin" if f < 8 else "pose", table="twist:%d" % (6 * (f + 1)))
        b.add("guides")
        b.pt()
        if f % 4 == 3:
            b.add(builds[f // 4][0], **builds[f // 4][1])
            b.add("tree")
    b.add("ppm")
    b.add("infos")
    return b.session()


def _session_t(hpt):
    """P's first forty steps on three triangles: the same calls, their legality decided again."""
    b = Builder(hpt, "T", "tiny3")
    for st in session("P", hpt).steps[:40]:
        kw = dict(st.kw)
        if st.kind == "refused":
            kw.pop("label")
            b.add(kw.pop("call"), **kw)
        else:
            b.add(st.kind, **kw)
    return b.session()


def _session_z(hpt):
    b = Builder(hpt, "Z", "none")
    calls = [("set_morphs", dict(morphs="four")), ("morph", dict(w=WEIGHTS[4][2])), ("set_parts", {}), ("pose", dict(table="turn:30")),
             ("set_skin", dict(skin="height")), ("skin", dict(table="twist:20")), ("update_triangles", dict(edit="base")),
             ("update_vertices_device", dict(edit="base")), ("rebuild", {}), ("rebuild_device", {}), ("rebuild_device_bounded", dict(depth="0")),
             ("update_rounds", dict(edit="moved")), ("keep_previous", {}), ("set_groups", dict(which="bend"))]
    for kind, kw in calls:
        b.add(kind, **kw)
    for kind in OBSERVATIONS:
        b.add(kind, **(dict(seed=21) if kind.startswith("probe") else dict(walk="default") if kind == "pt" else {}))
    for label in ("pose, no parts", "bounded, 31", "bounded, negative"):
        b.refuse(label)
    return b.session()


# A1 .. A6.  Seeds 4 and 5 were replaced by 9 and 23: with 1 .. 6 only A6 told mutant v apart and only A3 mutant viii
A_SEEDS = (1, 2, 3, 9, 23, 6)
A_NAMES = ["A%d" % (k + 1) for k in range(len(A_SEEDS))]
A_STEPS = 40


def _session_a(hpt, name):
    rng = np.random.default_rng(A_SEEDS[A_NAMES.index(name)])
    b = Builder(hpt, name, "bend")
    pick = lambda pool: pool[int(rng.integers(len(pool)))]
    vocabulary = STATE_KINDS + OBSERVATIONS + ("refused",)
    # the triangle-state kinds are drawn twice as often as the rest, pose, skin and morph five times: half of those draws find
    # no parts, skin or morphs and become refusals, and the chains that tell the models apart need several of them accepted
    p = np.array([5.0 if k in ("pose", "skin", "morph") else 2.0 if k in TRI_KINDS else 1.0 for k in vocabulary])
    p /= p.sum()
    while len(b.steps) < A_STEPS:
        kind = vocabulary[int(rng.choice(len(vocabulary), p=p))]
        if kind == "refused":
            labels = [lab for lab in REFUSALS if available(b.sd, b.model, lab)]
            b.refuse(pick(labels))
        else:
            kw = b.choose(kind, pick)
            if kw is not None:
                b.add(kind, **kw)
    return b.session()


NAMES = ["P", "K", "M1", "M2", "M3", "M4", "F", "T", "Z"] + A_NAMES
_SESSIONS = {}


def session(name, hpt):
    if name not in _SESSIONS:
        if name == "P":
            s = _session_p(hpt)
        elif name == "K":
            s = _session_k(hpt)
        elif name[0] == "M":
            s = _session_m(hpt, int(name[1:]))
        elif name == "F":
            s = _session_f(hpt)
        elif name == "T":
            s = _session_t(hpt)
        elif name == "Z":
            s = _session_z(hpt)
        else:
            s = _session_a(hpt, name)
        _SESSIONS[name] = s
    return _SESSIONS[name]


def is_change(st):
    """A state-changing or refused step: what the GPU half checks the whole handle after."""
    return st.kind in STATE_KINDS or st.kind == "refused"
