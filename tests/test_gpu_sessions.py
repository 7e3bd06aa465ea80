"""One long-lived handle across every integrator, on the MI355X: the sessions of session_cases.py run step by step on a
single hpt_scene (or fan-out, or the scene the one-shot wrappers keep) and every step is held to the CPU oracles' bytes.

The integrators share pass[0]'s path state and queues, one counter buffer laid out three ways, the accumulator, the work
counters, the own framebuffers and the render events, all grow-only and reached through views that every integrator
refreshes for itself; a test that opens a handle for one render sees none of it.  Here the size, depth, delta cap, tile,
samples per pass, flags and integrator change from step to step, up and down, and the repeated steps must give the bytes
of their first occurrence.  Statistics steps hold hpt_get_stats to "the last render only": zeros after photon mapping
and guides (which count into hpt_ppm_stats), the oracle's ray counts after a counting PT render.  The update steps
(sessions G, G_rounds, G_parallel, R4..R6) replace the records the handle holds; everything after them is the oracles'
result on the records in force, and the exported tree the host definition's refit of the builder's.

A mismatch names the session, the step, its record and the first differing value.  The `_device` steps run on a torch
side stream and are waited for before the next step (include/hpt.h, hpt_render_pt_device: work on one scene is ordered
only by the caller's streams).  tests/test_session_cases_cpu.py keeps the expected results lit and distinct."""
import ctypes as C
import re

import numpy as np
import pytest

import session_cases as sc
from test_gpu_ppm import _load

pytestmark = pytest.mark.gpu

PPM_COUNTS = ("photons", "photon_rays", "deposits", "hit_points", "direct_pixels")
GUIDE_KEYS = ("albedo", "normal", "position", "coverage")
TREE_KEYS = ("num_nodes", "num_tris", "bvh_depth", "num_rounds", "qorigin", "qscale", "qnodes", "tris")


@pytest.fixture(scope="module")
def orc(oracle_mod, tmp_path_factory):
    return sc.Oracles(oracle_mod, tmp_path_factory.mktemp("session_oracles"))


def _where(session, i):
    return "session %s, step %d, %s %r" % (session.name, i, session.steps[i].kind, session.steps[i].kw)


def _same(session, i, what, got, want):
    """Byte equality; on a mismatch the failure names the step and the first differing value (for an image [y, x, channel])."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes():
        return
    if got.shape != want.shape or got.dtype != want.dtype:
        pytest.fail("%s: %s is %s %s, expected %s %s" % (_where(session, i), what, got.dtype, got.shape, want.dtype, want.shape))
    bits = "u%d" % got.dtype.itemsize
    diff = np.argwhere(got.view(bits) != want.view(bits))
    at = tuple(int(v) for v in diff[0])
    pytest.fail("%s: %s differs in %d of %d values, first at %s: got %r, expected %r"
                % (_where(session, i), what, len(diff), got.size, at, got[at].item(), want[at].item()))


def _equal(session, i, what, got, want):
    assert got == want, "%s: %s is %r, expected %r" % (_where(session, i), what, got, want)


def _params(hpt, kw):
    p = hpt.make_params(seed=kw.get("seed", 1), sample_offset=kw.get("sample_offset", 0), max_delta=kw.get("max_delta", 0),
                        rank=kw.get("rank", 0), world=kw.get("world", 1), tile=kw.get("tile", 0),
                        samples_per_pass=kw.get("samples_per_pass", 0), flags=kw.get("flags", 0))
    p.reserved = kw.get("reserved", kw.get("budget", 0) << 1)
    return p


def _ptr(a):
    return np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


class Run:
    """One session on one handle."""

    def __init__(self, hpt, session, expected):
        self.hpt, self.session, self.expected = hpt, session, expected
        self.sd = self.cur = sc.current(session.scene)          # cur: the records the handle holds, replaced by the update steps
        self.L, self.sp, self.tr = self.sd["L"], self.sd["sp"], self.sd["tr"]
        self.states, self.gathered, self.results, self.side = {}, {}, [], None
        self.h = self.constants = None

    # -- the calls ---------------------------------------------------------------------------------------------------
    def pt(self, kw):
        return self.h.render_pt(sc.camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], kw["depth"], kw["spp"], _params(self.hpt, kw))

    def bdpt(self, kw):
        return self.h.render_bdpt(sc.bdpt_camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], kw["depth"], kw["light_depth"], kw["spp"], kw["spl"],
                                  _params(self.hpt, kw))

    def ppm(self, kw):
        return self.h.render_ppm(sc.camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], kw["depth"], kw["light_depth"], kw["spp"], kw["spl"],
                                 kw.get("radius", 0.05), _params(self.hpt, kw))

    def guides(self, kw):
        return self.h.render_guides(sc.camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], kw["spp"], _params(self.hpt, kw))

    def guides_null(self, kw):
        p = _params(self.hpt, kw)
        lib = self.hpt.load_library()
        rc = lib.hpt_render_guides(self.h._h, _ptr(sc.camera(self.sd, kw["W"], kw["H"])), kw["W"], kw["H"], kw["spp"], C.byref(p), None, None, None, None)
        if rc:
            raise self.hpt.HptError("hpt error %d: %s" % (rc, lib.hpt_last_error().decode("utf-8", "replace")))

    def sppm_create(self, kw):
        return self.h.sppm(sc.camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], kw["depth"], kw["light_depth"], kw["spl"], kw["radius"], kw["alpha"],
                           _params(self.hpt, kw))

    def side_stream(self):
        import torch
        if self.side is None:
            self.side = torch.cuda.Stream()
        return self.side

    def device_rank(self, kw):
        import torch
        if kw["group"] not in self.gathered:
            self.gathered[kw["group"]] = torch.zeros((sc.WORLD, sc.n_local(kw, sc.WORLD), 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
        row = self.gathered[kw["group"]][kw["rank"]]
        side = self.side_stream()
        self.h.render_pt_device(sc.camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], kw["depth"], kw["spp"],
                                _params(self.hpt, dict(kw, world=sc.WORLD)), row.data_ptr(), side.cuda_stream)
        side.synchronize()                                  # before anything else touches the scene
        return row.cpu().numpy()

    def untile(self, kw):
        import torch
        image = torch.empty((kw["H"], kw["W"], 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        side = self.side_stream()
        self.hpt.untile(self.gathered[kw["group"]].data_ptr(), image.data_ptr(), kw["W"], kw["H"], _params(self.hpt, dict(kw, world=sc.WORLD)), side.cuda_stream)
        side.synchronize()
        return image.cpu().numpy()

    def bdpt_wrapper(self, kw):
        lib = self.hpt.load_library()
        img = np.empty((kw["H"], kw["W"], 3), np.float32)
        z3 = (C.c_float * 3)()
        rc = lib.hpt_bdpt_render_wrapper(_ptr(self.L), len(self.L), _ptr(self.sp), len(self.sp), _ptr(self.tr), len(self.tr), z3, z3,
                                         _ptr(sc.bdpt_camera(self.sd, kw["W"], kw["H"])), img.ctypes.data_as(C.c_void_p), kw["W"], kw["H"],
                                         kw["light_depth"], kw["light_sample"], kw["depth"], kw["spp"], kw["spl"], C.c_int64(kw["seed"]))
        assert rc == 0, lib.hpt_last_error()
        return img

    # -- the steps ---------------------------------------------------------------------------------------------------
    def check_ppm_stats(self, i, want, counted, extra=()):
        st = self.h.ppm_stats()
        for k in PPM_COUNTS + (tuple(extra) if counted else ()):
            _equal(self.session, i, "hpt_ppm_stats." + k, st[k], want[k])

    def step(self, i):
        s, hpt = self.session, self.hpt
        st, e = s.steps[i], self.expected[i]
        k, kw, got = st.kind, st.kw, None
        if k in ("pt", "bdpt"):
            got = dict(image=getattr(self, k)(kw))
        elif k == "ppm":
            got = dict(image=self.ppm(kw))
            self.check_ppm_stats(i, e["stats"], kw.get("flags", 0) & sc.COUNT_WORK, sc.ppm_oracle.WORK)
        elif k == "guides":
            got = self.guides(kw)
            _equal(s, i, "hpt_ppm_stats.hit_points", self.h.ppm_stats()["hit_points"], e["hit_points"])
        elif k == "set_groups":
            order = self.sd["file_order"] if kw["which"] == "file" else [np.zeros(0, np.int32)] * 3
            self.h.set_groups(*order)
        elif k == "sppm_create":
            self.states[kw["name"]] = self.sppm_create(kw)
        elif k == "sppm_render":
            got = dict(image=self.states[kw["name"]].render(kw["passes"], kw.get("flags", 0)))
            self.check_ppm_stats(i, e["stats"], kw.get("flags", 0) & sc.COUNT_WORK, ("candidates", "accepted"))
        elif k == "sppm_reset":
            self.states[kw["name"]].reset()
        elif k == "sppm_state":
            got = self.states[kw["name"]].state()
            _equal(s, i, "passes", got["passes"], e["passes"])
        elif k == "sppm_destroy":
            self.states.pop(kw["name"]).close()
        elif k == "probe_closest":
            o, d, _ = sc.probe_rays(self.cur, kw["n"], kw["seed"])
            t, prim = self.h.trace_closest(o, d)
            got = dict(t=t, prim=prim)
        elif k == "probe_visibility":
            o, _, p2 = sc.probe_rays(self.cur, kw["n"], kw["seed"])
            got = dict(visible=self.h.trace_visibility(o, p2))
        elif k == "export_bvh":
            # the builder's tree while the handle holds the triangles it was created from (before any update, and after
            # an update back to them), else the definition's refit of that tree to the current triangles
            base = self.cur["edits"][0] == "base"
            host = hpt.export_bvh_host(self.L, self.sp, self.tr) if base else hpt.refit_bvh_host(self.L, self.sp, self.tr, self.cur["tr"])
            dev = self.h.export_bvh()
            for key in TREE_KEYS:
                _same(s, i, "exported " + key, dev[key], host[key])
        elif k in sc.UPDATES:
            self.cur = sc.after_update(self.cur, st)
            if k == "update_triangles":
                self.h.update_triangles(self.cur["tr"])
                info = self.h.update_info()
                for key in ("updates", "live_tris", "dead_tris"):
                    _equal(s, i, "hpt_update_info." + key, info[key], e[key])
            else:
                self.h.update_rounds(self.cur["L"], self.cur["sp"])
        elif k == "stats":
            self.check_stats(i, e)
        elif k == "refused":
            call = dict(pt=self.pt, bdpt=self.bdpt, ppm=self.ppm, guides=self.guides, guides_null=self.guides_null, sppm_create=self.sppm_create,
                        sppm_render=lambda a: self.states[a["name"]].render(a["passes"]),
                        update_triangles=lambda a: self.h.update_triangles(*sc.refused_update_args(self.cur, a)),
                        update_rounds=lambda a: self.h.update_rounds(*sc.refused_update_args(self.cur, a)))[kw["call"]]
            try:
                call(kw)
            except hpt.HptError as err:
                m = re.match(r"hpt error (\d+):", str(err))
                _equal(s, i, "error code (%s)" % err, int(m.group(1)) if m else None, e["code"])
            else:
                pytest.fail("%s: the call was accepted" % _where(s, i))
        elif k == "pt_device_rank":
            got = dict(local=self.device_rank(kw))
        elif k == "untile":
            got = dict(image=self.untile(kw))
        elif k == "pt_wrapper":
            tr = sc.changed_triangles(self.tr) if kw.get("changed") else self.tr
            got = dict(image=hpt.pt_render_wrapper(self.L, self.sp, tr, sc.camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], kw["depth"], kw["spp"], seed=kw["seed"]))
        elif k == "bdpt_wrapper":
            got = dict(image=self.bdpt_wrapper(kw))
        elif k == "ppm_wrapper":
            got = dict(image=hpt.ppm_render_wrapper(self.L, self.sp, self.tr, sc.camera(self.sd, kw["W"], kw["H"]), kw["W"], kw["H"], self.sd["lo"], self.sd["hi"],
                                                    kw["light_depth"], kw["spl"], kw["depth"], 1, seed=kw["seed"]))
        else:
            raise ValueError(k)
        if got is not None:
            for key in sorted(got):
                if isinstance(got[key], np.ndarray):
                    _same(s, i, key, got[key], e[key])
            if st.repeat_of is not None:
                for key in sorted(got):
                    if isinstance(got[key], np.ndarray):
                        _same(s, i, "%s of the repeat of step %d" % (key, st.repeat_of), got[key], self.results[st.repeat_of][key])
        self.results.append(got)

    def check_stats(self, i, e):
        """hpt_get_stats describes the last render only: the table's exact fields, a total time, and the scene constants
        the handle had when it was opened."""
        st = self.h.stats()
        for f, want in e["equal"].items():
            _equal(self.session, i, "hpt_stats." + f, st[f], want)
        assert st["ms_total"] > 0, "%s: ms_total is %r" % (_where(self.session, i), st["ms_total"])
        for f in sc.CONSTANTS:
            _equal(self.session, i, "hpt_stats." + f, st[f], self.constants[f])

    def run(self):
        s, hpt = self.session, self.hpt
        try:
            if s.handle == "scene":
                self.h = hpt.Scene(self.L, self.sp, self.tr)
                self.constants = {f: self.h.stats()[f] for f in sc.CONSTANTS}
                assert self.constants["n_tris"] == len(self.tr) and self.constants["bvh_nodes"] > 0
            elif s.handle == "multi":
                self.h = hpt.MultiScene(self.L, self.sp, self.tr, device_ids=[0] * sc.WORLD, exchange=1)
                assert self.h.num_devices == sc.WORLD
            else:
                hpt.wrapper_cache_clear()
            for i in range(len(s.steps)):
                self.step(i)
        finally:
            for z in self.states.values():
                z.close()
            if self.h is not None:
                self.h.close()
            if s.handle == "wrappers":
                hpt.wrapper_cache_clear()


def _run(hpt, orc, name):
    session = sc.session(name)
    Run(hpt, session, sc.expected(orc, session)).run()


def test_the_table_renders_the_scenes_of_the_other_suites(sio):
    """The table's input.txt records and camera are the ones test_gpu_ppm's builder hands to the PPM, SPPM and guide tests."""
    L, sp, tr, cam = _load(sio, "input", 48, 40)
    sd = sc.scene("input")
    assert L.tobytes() == sd["L"].tobytes() and sp.tobytes() == sd["sp"].tobytes() and tr.tobytes() == sd["tr"].tobytes()
    assert np.ascontiguousarray(cam).tobytes() == np.ascontiguousarray(sc.camera(sd, 48, 40)).tobytes()


def test_session_a_frames(hpt, orc):
    """Also: a fresh handle whose first render is PPM reports zeros, not the never-written work counters."""
    _run(hpt, orc, "A")
    _run(hpt, orc, "A_fresh")


def test_session_b_flags(hpt, orc):
    _run(hpt, orc, "B")


def test_session_c_two_progressive_states(hpt, orc):
    _run(hpt, orc, "C")


def test_session_d_refusals(hpt, orc):
    _run(hpt, orc, "D")


def test_session_e_fan_out(hpt, orc):
    _run(hpt, orc, "E")


def test_session_f_one_shot_wrappers(hpt, orc):
    _run(hpt, orc, "F")


def test_session_g_a_scene_over_time(hpt, orc):
    """Updates between rounds that grow and shrink the workspace and run every flag; two progressive states without and
    with a reset; a rank group with an update between its ranks; every update refusal; the builder's bytes at the end."""
    _run(hpt, orc, "G")


def test_session_g_rounds(hpt, orc):
    _run(hpt, orc, "G_rounds")


def test_session_g_parallel_light(hpt, orc):
    """A progressive state under a parallel light across an update: stale bounds without a reset, the new scene's bounds
    after one (hpt_sppm_reset re-reads the bounds the state was created without)."""
    _run(hpt, orc, "G_parallel")


@pytest.mark.parametrize("seed", sc.R_SEEDS)
def test_random_session(hpt, orc, seed):
    _run(hpt, orc, "R%d" % seed)
