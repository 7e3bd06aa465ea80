"""Morph targets on the host alone (morph_cases.py): hpt_morph_host, the definition, held to the numpy restatement of
morph_oracle.py byte for byte on every morph step, and composed with hpt_pose_host / hpt_skin_host to the expected records
of every step; the table held to its own conditions (every step changes the image, so a structure left stale cannot pass
the GPU half, tests/test_gpu_morph.py; `order` holds corners whose sum taken in descending target order has other bits and
`contract` corners that a fused multiply-add rounds differently, so a kernel with either mistake cannot pass; keep,
inactive NaN targets, negative, denormal and infinite weights and dead triangles are reached); the refusals that need no
handle, each with its message; and the chains of morphs of die-and-return and all-4096 in a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import morph_cases as mc
import morph_oracle as mo
import pose_oracle as po
import refit_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
SCANNED = [n for n in mc.NAMES if n != "grid-stride"]               # (grid-stride is rendered by the walk alone: see morph_cases)
MORPHS = mc.morph_steps()
MORPH_IDS = ["%s-%d" % s for s in MORPHS]
GEOMETRY = mc.all_geometry_steps()
GEOMETRY_IDS = ["%s-%d" % s for s in GEOMETRY]
U32 = np.uint32


def _same_bytes(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        a, b = po.verts_of(got).view(U32), po.verts_of(want).view(U32)
        at = np.argwhere(a != b)
        pytest.fail("%s: %d vertex words differ, first at %s: got %08x, expected %08x" % (what, len(at), at[0].tolist(), a[tuple(at[0])], b[tuple(at[0])]))


# ---- the definition against its restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,step", MORPHS, ids=MORPH_IDS)
def test_morph_host_equals_the_oracle(hpt, name, step):
    d = mc.data(name)
    st = mc.expected(name)[step]
    got = hpt.morph_host(st.rest, *st.targets, d.steps[step][1])
    _same_bytes("%s step %d" % (name, step), got, st.morphed)
    for f in ("mtl_old", "mtl", "id"):                               # only vertices move
        assert got[f].tobytes() == d.tr[f].tobytes(), f


@pytest.mark.parametrize("name,step", GEOMETRY, ids=GEOMETRY_IDS)
def test_the_host_chain_equals_the_expected_records(hpt, name, step):
    """hpt_morph_host, then hpt_pose_host or hpt_skin_host with the deformer's last table: the records of every step."""
    _same_bytes("%s step %d" % (name, step), mc.host_chain(hpt, mc.expected(name)[step]), mc.expected(name)[step].tr)


def test_zero_weights_of_either_sign_return_the_inputs_bytes(hpt):
    d = mc.data("zero")
    bits = po.verts_of(d.tr).view(U32)
    assert bits[0, 1, 0] == 0x80000000 and bits[11, 2, 1] == 0x7FC12345
    t = d.steps[0][1:]
    assert np.isnan(t[2][t[0][1]:t[0][2]]).any()                   # NaN deltas on the walls, the -0 and the payload among them
    assert {1, 35} <= set(t[1][t[0][1]:t[0][2]].tolist())          # corner 1 of triangle 0, corner 2 of triangle 11
    for step in (1, 2):
        wts = d.steps[step][1]
        assert not mo.active(wts).any()
        assert hpt.morph_host(d.tr, *t, wts).tobytes() == d.tr.tobytes(), step
    assert (d.steps[2][1].view(U32) == 0x80000000).sum() == 2
    got = po.verts_of(hpt.morph_host(d.tr, *t, d.steps[3][1])).view(U32)
    assert np.array_equal(got[:mc.NWALL], bits[:mc.NWALL])          # the walls keep -0 and the payload while the sphere bulges
    assert not np.array_equal(got[mc.NWALL:], bits[mc.NWALL:])
    assert mc.records("die-and-return", 7)[2].tobytes() == mc.data("die-and-return").tr.tobytes()      # all back is the base
    assert mc.records("no-entries", 1)[2].tobytes() == mc.data("no-entries").tr.tobytes()


def test_exact_is_exact():
    d = mc.data("exact")
    got = po.verts_of(mc.records("exact", 1)[2])[mc.NWALL:].astype(np.float64)
    assert np.array_equal(got, po.verts_of(d.tr)[mc.NWALL:].astype(np.float64) * 0.5)


# ---- the table ---------------------------------------------------------------------------------------------------------

def test_the_table_has_the_cases_the_suite_is_about():
    assert mc.NAMES == ["zero", "exact", "order", "contract", "die-and-return", "sparse", "no-entries", "all-4096", "one-each",
                        "tiny-1", "tiny-2", "tiny-3", "edges-85", "edges-86", "grid-stride", "with-parts", "with-skin", "recapture",
                        "tris-between", "swap", "twice"]
    assert [len(mc.data(n).tr) for n in ("tiny-1", "tiny-2", "tiny-3", "edges-85", "edges-86", "zero")] == [1, 2, 3, 85, 86, 276]
    assert [(3 * n) % 256 for n in mc.EDGE_COUNTS] == [255, 2]      # one lane per corner, workgroups of 256
    assert len(mc.data("grid-stride").tr) == mc.N_STRIDE and 3 * mc.N_STRIDE == 2048 * 256 + 1
    assert mc.data("grid-stride").steps[0][2][-1] == 3 * mc.N_STRIDE - 1         # the second trip's corner is morphed
    for name, targets, entries in (("all-4096", 4096, 4096), ("one-each", 4096, 4096), ("no-entries", 2, 0), ("sparse", 4, 2)):
        tb, ec, ed = mc.data(name).steps[0][1:]
        assert (len(tb) - 1, len(ec), len(ed)) == (targets, entries, entries), name
    assert set(mc.data("all-4096").steps[0][2].tolist()) == {1} and len(set(mc.data("one-each").steps[0][2].tolist())) == 4096
    tb, ec, _ = mc.data("sparse").steps[0][1:]
    assert tb.tolist() == [0, 0, 1, 2, 2] and ec.tolist() == [0, 3 * 276 - 1]
    assert [s[0] for s in mc.data("with-parts").steps] == ["morphs", "parts", "morph", "pose", "morph", "pose"]
    assert [s[0] for s in mc.data("with-skin").steps] == ["set", "morphs", "morph", "skin", "morph", "skin"]
    assert [s[0] for s in mc.data("recapture").steps] == ["morphs", "morph", "parts", "pose", "morph"]
    assert [s[0] for s in mc.data("tris-between").steps] == ["morphs", "morph", "tris", "morph", "dverts", "morph"]
    assert [s[0] for s in mc.data("swap").steps] == ["morphs", "parts", "pose", "morph", "set", "morph", "skin"]
    assert [s[0] for s in mc.data("twice").steps] == ["morphs", "morph", "morphs", "morph"]
    for (name, step), n in mc.N_DEAD.items():
        assert int(rc.dead(mc.records(name, step)[2]).sum()) == n, (name, step)
    for name in mc.NAMES:
        d = mc.data(name)
        for step in range(len(d.steps)):
            tr = mc.records(name, step)[2]
            assert len(tr) == len(d.tr)
            for f in ("mtl_old", "mtl", "id"):
                assert tr[f].tobytes() == d.tr[f].tobytes(), (name, step, f)


def test_the_table_reaches_the_weights_and_the_captures_the_issue_names():
    wts = np.concatenate([mc.data(n).steps[s][1] for n, s in MORPHS])
    bits = wts.view(U32)
    tiny = np.finfo(np.float32).tiny
    assert (bits == 0).any() and (bits == 0x80000000).any() and (wts < 0).any() and np.isinf(wts).any()
    assert ((np.abs(wts) < tiny) & (wts != 0)).any() and (wts == np.float32(1e30)).any()
    # die-and-return: NaN deltas that are named under a zero weight (no effect, the walls' among them) and under 1 (dead)
    d = mc.data("die-and-return")
    tb, ec, ed = d.steps[0][1:]
    assert np.isnan(ed[tb[1]:tb[2]]).any(axis=1).all() and (ec[tb[1]:tb[2]] < 6).sum() == 6
    assert not rc.dead(mc.records("die-and-return", 1)[2]).any() and rc.dead(mc.records("die-and-return", 2)[2])[:2].all()
    # recapture: after set_parts the rest pose is the morphed geometry, M is R and the weights are zero
    st = mc.expected("recapture")
    assert st[2].rest.tobytes() == st[1].tr.tobytes() == st[2].morphed.tobytes() and st[2].rest.tobytes() != mc.data("recapture").tr.tobytes()
    assert not st[2].weights.any() and st[2].table is None and st[2].targets is st[1].targets
    # swap: set_skin replaces the parts, keeps the targets and captures
    st = mc.expected("swap")
    assert st[3].deformer[0] == "parts" and st[4].deformer[0] == "skin" and st[4].targets is st[3].targets
    assert st[4].rest.tobytes() == st[3].tr.tobytes() and not st[4].weights.any()
    # tris-between: the update's records are the rest pose of the next morph
    st = mc.expected("tris-between")
    assert st[2].rest.tobytes() == st[2].tr.tobytes() and st[3].rest is st[2].rest and st[3].tr.tobytes() != st[1].tr.tobytes()
    # twice: the second set_morphs captures the morphed geometry
    st = mc.expected("twice")
    assert st[2].rest.tobytes() == st[1].tr.tobytes() and len(st[2].targets[0]) == 4


@pytest.mark.parametrize("name,step", mc.all_geometry_steps(SCANNED), ids=["%s-%d" % s for s in mc.all_geometry_steps(SCANNED)])
def test_every_step_changes_the_image(hpt, oracle_mod, name, step):
    """... against the step before, so that a device structure left stale by a morph cannot render the step's bytes."""
    now, before = mc.scan(oracle_mod, name, step, hpt)[0], mc.scan(oracle_mod, name, step - 1, hpt)[0]
    share = rc.changed_share(now, before)
    print("%s step %d: %.1f %% of the pixels change" % (name, step, 100 * share))
    assert np.isfinite(now).all()
    if (name, step) in mc.SAME_AS_BEFORE:
        assert share == 0.0
    else:
        assert share > 0.0


def test_order_and_contract_tell_the_two_mistakes_apart():
    """`order`: corners whose sum has other bits when the targets are taken in descending order.  `contract`: corners whose
    sum has other bits when w * d + acc is one fused multiply-add.  Either mistake in the kernel changes expected bytes."""
    for name, kw in (("order", dict(descending=True)), ("contract", dict(fuse=True))):
        d = mc.data(name)
        total = 0
        for step in range(1, len(d.steps)):
            st = mc.expected(name)[step]
            v = po.verts_of(st.rest)
            plain = mo.raw(v, *st.targets, st.weights).view(U32)
            other = mo.raw(v, *st.targets, st.weights, **kw).view(U32)
            differ = int((plain != other).any(axis=-1).sum())
            print("%s step %d: %d corners differ with %s" % (name, step, differ, kw))
            total += differ
            if differ:
                assert mo.morph(st.rest, *st.targets, st.weights, **kw).tobytes() != st.morphed.tobytes()
        assert total > 0, name
    # ... and each case is blind to the other mistake's opposite: the plain variants agree with themselves
    st = mc.expected("order")[1]
    assert mo.morph(st.rest, *st.targets, st.weights).tobytes() == st.morphed.tobytes()


# ---- the refusals that need no handle --------------------------------------------------------------------------------

def _refused(hpt, call, *words):
    with pytest.raises(hpt.HptError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith("hpt error 1:"), msg
    for word in words:
        assert word in msg, msg


def test_refusals_without_a_device(hpt):
    lib = hpt.load_library()
    d = rc.data("tiny-3")
    tr = np.ascontiguousarray(d.tr)
    out = tr.copy()
    tb, ec, ed = mc.targets(([0, 4, 8], np.full((3, 3), 0.1)), mc.EMPTY, ([2, 3], np.full((2, 3), -0.1)))
    wts = mc.w(1.0, 1.0, 1.0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    host = lambda tb_=tb, ec_=ec, ed_=ed, w_=wts, nt=3, ne=None, ntg=None, tr_=tr, out_=out: lib.hpt_morph_host(
        vp(tr_) if tr_ is not None else None, nt, vp(tb_) if tb_ is not None else None, vp(ec_) if ec_ is not None else None,
        vp(ed_) if ed_ is not None else None, len(ec) if ne is None else ne, len(tb) - 1 if ntg is None else ntg,
        vp(w_) if w_ is not None else None, vp(out_) if out_ is not None else None)

    def said(rc_, *words):
        msg = lib.hpt_last_error()
        assert rc_ == 1, msg
        for word in words:
            assert word.encode() in msg, msg

    def edited(a, at, value):
        a = a.copy(); a[at] = value
        return a
    said(lib.hpt_scene_set_morphs(None, vp(tb), vp(ec), vp(ed), len(ec), 3, 3), "null scene")
    said(lib.hpt_scene_morph(None, vp(wts), 3), "null scene")
    said(host(ntg=0), "morph targets must lie in [1, 4096]", "0 was given")
    said(host(ntg=4097), "morph targets must lie in [1, 4096]", "4097 was given")
    said(host(ne=-1), "negative morph entry count")
    said(host(nt=-1), "negative triangle count")
    said(host(tb_=None), "null target_begin")
    said(host(ec_=None), "null morph entry array")
    said(host(ed_=None), "null morph entry array")
    said(host(w_=None), "null weight array")
    said(host(tr_=None), "null triangle array")
    said(host(out_=None), "null triangle array")
    said(host(tb_=edited(tb, 0, 1)), "target_begin[0] must be 0", "it is 1")
    said(host(tb_=edited(tb, 2, 2)), "target_begin decreases at target 1", "2 follows 3")
    said(host(ne=4), "target_begin[3] must be the number of entries, 4", "it is 5")
    said(host(tb_=edited(tb, 3, 4)), "target_begin[3] must be the number of entries, 5", "it is 4")
    said(host(ec_=edited(ec, 2, 9)), "corner 9 of target 0 (entry 2) is not one of the 9 corners")
    said(host(ec_=edited(ec, 3, -1)), "corner -1 of target 2 (entry 3) is not one of the 9 corners")
    said(host(ec_=edited(ec, 1, 0)), "corners of target 0 are not strictly ascending", "entry 1 names corner 0 after corner 0")
    said(host(ec_=edited(ec, 4, 1)), "corners of target 2 are not strictly ascending", "entry 4 names corner 1 after corner 2")
    # the first one in entry order is named
    said(host(ec_=edited(edited(ec, 4, 1), 1, 0)), "target 0", "entry 1")
    # a descending corner across two targets is no fault: entry 3 (target 2) names corner 2 after target 0's corner 8
    assert ec[2] == 8 and ec[3] == 2
    _refused(hpt, lambda: hpt.morph_host(tr, tb, ec, ed[:-1], wts), "three floats per entry")
    _refused(hpt, lambda: hpt.morph_host(tr, tb, ec, ed, wts[:2]), "one weight per target")
    _refused(hpt, lambda: hpt.morph_host(tr[:1], tb, ec, ed, wts), "is not one of the 3 corners")
    assert out.tobytes() == tr.tobytes()                          # a refused call writes nothing
    # weights and deltas are not validated
    got = hpt.morph_host(tr, tb, ec, edited(ed, (0, 0), float("nan")), mc.w(float("inf"), -1.0, float("nan")))
    assert (po.verts_of(got).view(U32)[0, 0] == 0x7FC00000).all()
    # zero triangles with zero entries, and a morph in place
    none = np.zeros(2, np.int32)
    assert lib.hpt_morph_host(None, 0, vp(none), None, None, 0, 1, vp(wts), None) == 0
    assert host(tr_=out) == 0
    _same_bytes("in place", out, mo.morph(tr, tb, ec, ed, wts))
    assert out.tobytes() != tr.tobytes()


# ---- undefined behaviour: the chains of morphs, under the sanitizers -----------------------------------------------

SAN_FLAGS = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def morph_check(tmp_path_factory):
    """tests/morph_check.cpp + csrc/scene_build.cpp as one stand-alone program with the sanitizers in, compiled the way
    test_skin_cpu.py compiles skin_check.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("morph_check") / "morph_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread"] + SAN_FLAGS + static
                          + ["-I", CSRC, "-o", exe, os.path.join(HERE, "morph_check.cpp"), os.path.join(CSRC, "scene_build.cpp")])
    return exe


def _fnv(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("name", ["die-and-return", "all-4096", "sparse"])
def test_the_chain_of_morphs_is_clean_under_the_sanitizers(hpt, morph_check, tmp_path, name):
    """The program morphs the base records step after step -- by the caller's layout, in place, and by the per-corner walk
    of the device's layout -- and refits ONE HostScene to each; every step's records are the oracle's and every tree the one
    hpt_bvh_refit_host gives from the base scene directly."""
    d = mc.data(name)
    assert d.steps[0][0] == "morphs"
    tb, ec, ed = d.steps[0][1:]
    steps = [s for s in range(1, len(d.steps)) if d.steps[s][0] == "morph"]
    assert len(steps) == len(d.steps) - 1
    rec = str(tmp_path / "records.bin")
    L, sp, tr = (np.ascontiguousarray(a) for a in (d.L, d.sp, d.tr))
    with open(rec, "wb") as f:
        f.write(np.array([len(L), len(sp), len(tr), len(tb) - 1, len(ec), len(steps)], np.int32).tobytes())
        f.write(L.tobytes()); f.write(sp.tobytes()); f.write(tr.tobytes())
        f.write(np.ascontiguousarray(tb, np.int32).tobytes())
        f.write(np.ascontiguousarray(ec, np.int32).tobytes())
        f.write(np.ascontiguousarray(ed, np.float32).tobytes())
        for s in steps:
            f.write(np.ascontiguousarray(d.steps[s][1], np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([morph_check, rec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    assert b"runtime error" not in p.stderr and b"Sanitizer" not in p.stderr, p.stderr.decode(errors="replace")[-3000:]
    lines = [dict(kv.split("=") for kv in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert [int(o["step"]) for o in lines] == [-1] + list(range(len(steps)))
    for o, s in zip(lines, [-1] + steps):
        bvh, want = mc.tree(hpt, name, s), np.ascontiguousarray(mc.records(name, s)[2])
        assert int(o["records_fnv"], 16) == _fnv(want.tobytes()), s
        assert (int(o["nodes"]), int(o["tris"]), int(o["depth"])) == (bvh["num_nodes"], bvh["num_tris"], bvh["bvh_depth"]), s
        assert int(o["qnodes_fnv"], 16) == _fnv(bvh["qnodes"].tobytes()) and int(o["tris_fnv"], 16) == _fnv(bvh["tris"].tobytes()), s
        assert int(o["grid_fnv"], 16) == _fnv(bvh["qscale"].tobytes(), _fnv(bvh["qorigin"].tobytes())), s
        if s >= 0:
            assert int(o["dead"]) == int(rc.dead(want).sum()), s
