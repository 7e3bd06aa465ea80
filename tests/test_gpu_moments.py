"""The temporal variance on the MI355X: a history with HPT_HISTORY_MOMENTS against the numpy oracle
(tests/moments_oracle.py) over the whole case table (tests/moments_cases.py) -- mean, length, second moment, the variance
image and the counts, bit for bit and integer for integer, every caller image a view of one arena between sentinel bands;
a plain history beside it; a plain and a moments history on two streams; the refusals that need a live object; the chain
render -> guides -> advance -> length -> estimate -> hpt_history_variance in place -> guided run on the project's scene
against the chain of the oracles; and pt_cli --temporal-variance.

Bits of a NaN: IEEE 754 leaves the sign and payload of a NaN that an operation produces to the implementation (x86 gives
inf - inf the sign bit, the GPU does not), so where the oracle's mean or second moment is NaN the device's must be a NaN, and
every other value must have the oracle's bits.  Only the non_finite cases hold any; the variance image never does."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guided_oracle as go
import history_cases as hc
import moments_cases as mc
from conftest import GOLDEN, ROOT
from test_moments_cpu import chain_inputs, cpu_chain

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -7.25
BAND = 19          # floats between two images: no image starts on a 16-byte boundary by design
FRAME, NORMAL, POSITION, COVERAGE, MEAN, FALLBACK, VARIANCE = range(7)


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def glib(tmp_path_factory):
    import guides_oracle
    return guides_oracle.build(tmp_path_factory.mktemp("guides_oracle"))


def _same(got, want, what):
    """The oracle's bits; a NaN where the oracle has a NaN."""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    assert not bad.any(), (what, "%d of %d values differ" % (int(bad.sum()), bad.size), np.argwhere(bad)[:4].tolist())


class Arena:
    """frame | normal | position | coverage | mean | fallback | variance, BAND sentinels before, between and after, in one
    device tensor."""

    def __init__(self, torch, W, H):
        self.torch, n = torch, W * H
        self.off, at = [], BAND
        for s in (3 * n, 3 * n, 3 * n, n, 3 * n, 3 * n, 3 * n):
            self.off.append((at, s))
            at += s + BAND
        assert sum(1 for lo, _ in self.off if lo % 4) >= 4
        self.host = np.full(at, SENTINEL, f32)
        self.dev = torch.full((at,), SENTINEL, dtype=torch.float32, device="cuda")

    def view(self, k):
        lo, s = self.off[k]
        return self.dev[lo:lo + s]

    def load(self, parts):
        """parts[k] (or None: sentinels) into image k."""
        for k, a in enumerate(parts):
            lo, s = self.off[k]
            self.host[lo:lo + s] = SENTINEL if a is None else np.asarray(a, f32).reshape(-1)
        self.dev.copy_(self.torch.from_numpy(self.host))
        self.torch.cuda.synchronize()

    def check(self, written):
        """written: {image: expected content}.  Every other float is as it was loaded."""
        got = self.dev.cpu().numpy()
        want = self.host.copy()
        for k, a in written.items():
            lo, s = self.off[k]
            want[lo:lo + s] = np.asarray(a, f32).reshape(-1)
        assert got.tobytes() == want.tobytes(), (sorted(written), int((got.view(np.uint32) != want.view(np.uint32)).sum()))


def _run_device(hpt, torch, case, stream=0):
    """(moments, plain): per advance what moments_cases.run_oracle returns, from a history with moments, and
    (mean, length, kept, restarted, frames) from a plain one fed the same frames."""
    W, H = mc.size_of(case)
    arena = Arena(torch, W, H)
    pattern = mc.pattern(W, H)
    out, plain_out = [], []
    with hpt.History(W, H, moments=True) as h, hpt.History(W, H) as plain:
        for step in case["steps"]:
            if step[0] == "reset":
                h.reset(stream=stream)
                plain.reset(stream=stream)
                continue
            a = step[1]
            g = a["guides"]
            mode = case["fallback"]
            arena.load([a["frame"], g["normal"] if g else None, g["position"] if g else None, g["coverage"] if g else None, None,
                        pattern if mode == "image" else None, pattern if mode == "in_place" else None])
            kw = dict(normal=arena.view(NORMAL), position=arena.view(POSITION), coverage=arena.view(COVERAGE)) if g else {}
            params = hpt.make_history_params(**a["params"]) if a["params"] else None
            mean_at = FRAME if a["in_place"] else MEAN
            plain.advance(a["camera"], arena.view(FRAME), params=params, stream=stream, **kw)      # no mean-out: reads only
            h.advance(a["camera"], arena.view(FRAME), params=params, mean_out=arena.view(mean_at), stream=stream, **kw)
            m, r = h.metrics(), h.read()
            arena.check({mean_at: r["mean"]})
            fallback = arena.view(FALLBACK) if mode == "image" else arena.view(VARIANCE) if mode == "in_place" else None
            h.variance(arena.view(VARIANCE), fallback=fallback, min_length=case["min_length"], stream=stream)
            torch.cuda.synchronize()
            lo, s = arena.off[VARIANCE]
            var = arena.dev[lo:lo + s].cpu().numpy().reshape(H, W, 3)
            arena.check({mean_at: r["mean"], VARIANCE: var})          # nothing but the output changed, the fallback image included
            r2 = h.read()
            assert all(r2[k].tobytes() == r[k].tobytes() for k in ("mean", "length", "q")) and h.metrics() == m      # a pure map
            out.append(dict(mean=r["mean"], length=r["length"], q=r["q"], variance=var, kept=m["kept"], restarted=m["restarted"], frames=m["frames"]))
            pm, pr = plain.metrics(), plain.read()
            assert "q" not in pr
            plain_out.append((pr["mean"], pr["length"], pm["kept"], pm["restarted"], pm["frames"]))
    return out, plain_out


@pytest.fixture(scope="module")
def device_results(hpt, torch):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run_device(hpt, torch, mc.CASES[name])
        return cache[name]
    return get


@pytest.fixture(scope="module")
def expected():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mc.run_oracle(mc.CASES[name])
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_case_equals_the_oracle(device_results, expected, name):
    got, want = device_results(name)[0], expected(name)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g["kept"], g["restarted"], g["frames"]) == (w["kept"], w["restarted"], w["frames"]), (name, k)
        if "non_finite" not in name:
            assert not np.isnan(w["mean"]).any() and not np.isnan(w["q"]).any(), (name, k)
        _same(g["mean"], w["mean"], (name, k, "mean"))
        _same(g["q"], w["q"], (name, k, "q"))
        assert g["length"].tobytes() == w["length"].tobytes(), (name, k, "length")
        assert not np.isnan(w["variance"]).any()
        assert g["variance"].tobytes() == w["variance"].tobytes(), (name, k, "variance", int((g["variance"].view(np.uint32) != w["variance"].view(np.uint32)).sum()))


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_plain_history_beside_it_has_the_same_mean_length_and_counts(device_results, name):
    moments, plain = device_results(name)
    assert len(moments) == len(plain)
    for k, (m, p) in enumerate(zip(moments, plain)):
        assert m["mean"].tobytes() == p[0].tobytes() and m["length"].tobytes() == p[1].tobytes(), (name, k)      # bytes: the devices' own NaNs agree
        assert (m["kept"], m["restarted"], m["frames"]) == p[2:], (name, k)


def test_plain_and_moments_history_of_different_sizes_on_two_streams(hpt, torch):
    names = ("size_67x3", "orbit_5")                             # the first on a plain history, the second with moments
    cases = [mc.CASES[n] for n in names]
    sizes = [mc.size_of(c) for c in cases]
    want = [mc.run_oracle(c) for c in cases]
    steps = [c["steps"] for c in cases]
    assert cases[1]["fallback"] == "image"
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams[0].cuda_stream != streams[1].cuda_stream != 0
    hist = [hpt.History(*sizes[0]), hpt.History(*sizes[1], moments=True)]
    dev = [[{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(s[1]["guides"], frame=s[1]["frame"]).items()} for s in st] for st in steps]
    means = [[torch.full((wh[1], wh[0], 3), SENTINEL, dtype=torch.float32, device="cuda") for _ in st] for st, wh in zip(steps, sizes)]
    variances = [torch.full((sizes[1][1], sizes[1][0], 3), SENTINEL, dtype=torch.float32, device="cuda") for _ in steps[1]]
    pattern = torch.from_numpy(mc.pattern(*sizes[1])).cuda()
    torch.cuda.synchronize()
    try:
        counts = [[], []]
        for k in range(max(len(s) for s in steps)):
            for i in (0, 1):
                if k < len(steps[i]):
                    d = dev[i][k]
                    hist[i].advance(steps[i][k][1]["camera"], d["frame"], d["normal"], d["position"], d["coverage"], mean_out=means[i][k],
                                    stream=streams[i].cuda_stream)
                    if i == 1:
                        hist[1].variance(variances[k], fallback=pattern, min_length=cases[1]["min_length"], stream=streams[1].cuda_stream)
            for i in (0, 1):
                if k < len(steps[i]):
                    m = hist[i].metrics()
                    counts[i].append((m["kept"], m["restarted"], m["frames"]))
        for i in (0, 1):
            streams[i].synchronize()
            assert counts[i] == [(w["kept"], w["restarted"], w["frames"]) for w in want[i]], names[i]
            for k, w in enumerate(want[i]):
                assert means[i][k].cpu().numpy().tobytes() == w["mean"].tobytes(), (names[i], k)
        for k, w in enumerate(want[1]):
            assert variances[k].cpu().numpy().tobytes() == w["variance"].tobytes(), k
        r = hist[1].read()
        assert r["q"].tobytes() == want[1][-1]["q"].tobytes() and r["length"].tobytes() == want[1][-1]["length"].tobytes()
        assert "q" not in hist[0].read()
    finally:
        for h in hist:
            h.close()


def test_refusals_on_a_live_object_enqueue_nothing(hpt, torch):
    lib = hpt.load_library()
    lib.hpt_history_variance.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    W, H = 5, 3
    n = W * H * 3
    cam = hc.camera(W, H)
    buf = torch.full((6 * n,), SENTINEL, dtype=torch.float32, device="cuda")
    frame = torch.from_numpy(hc.frame(hc.guides(cam, W, H), 3)).cuda()
    out, fb = buf[:n], buf[n:2 * n]
    with hpt.History(W, H) as plain:
        plain.advance(cam, frame)
        with pytest.raises(hpt.HptError, match="hpt error 1:.*without HPT_HISTORY_MOMENTS"):
            plain.variance(out, fallback=fb)
        q = np.zeros(n, f32)
        assert lib.hpt_history_read_moments(plain._h, q.ctypes.data_as(C.c_void_p)) == 1 and b"without HPT_HISTORY_MOMENTS" in lib.hpt_last_error()
    with hpt.History(W, H, moments=True) as h:
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before the first"):
            h.variance(out, fallback=fb)
        for k in range(4):
            h.advance(cam, frame)
        before, metrics = h.read(), h.metrics()
        assert (before["length"] == 4).all()
        nan = float("nan")
        for kw, word in ((dict(min_length=1.0), "min_length"), (dict(min_length=nan), "min_length"), (dict(min_length=-2.0), "min_length"),
                         (dict(fallback=buf[1:1 + n]), "must not overlap"), (dict(fallback=buf[n - 1:2 * n - 1]), "must not overlap")):
            args = dict(fallback=fb)
            args.update(kw)
            with pytest.raises(hpt.HptError, match="hpt error 1:.*" + word):
                h.variance(out, **args)
        assert lib.hpt_history_variance(h._h, None, 0.0, None, None) == 1 and b"null variance" in lib.hpt_last_error()
        assert lib.hpt_history_read_moments(h._h, None) == 1 and b"null moments" in lib.hpt_last_error()
        if torch.cuda.device_count() > 1:
            torch.cuda.set_device(1)
            try:
                with pytest.raises(hpt.HptError, match="hpt error 1:.*another device"):
                    h.variance(out, fallback=fb)
            finally:
                torch.cuda.set_device(0)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == f32(SENTINEL)).all()
        after = h.read()
        assert all(after[k].tobytes() == before[k].tobytes() for k in ("mean", "length", "q")) and after["frames"] == 4 and h.metrics() == metrics
        h.variance(out)                                                  # the call that is not refused writes: n = 4 everywhere
        torch.cuda.synchronize()
        assert not (buf[:n].cpu().numpy() == f32(SENTINEL)).any() and (buf[n:].cpu().numpy() == f32(SENTINEL)).all()
        h.reset()
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before the first"):
            h.variance(out)
        r = h.read()
        assert r["frames"] == 0 and not r["q"].any() and not r["mean"].any()
    for flags in (2, 5):
        bad = C.c_void_p()
        assert lib.hpt_history_create_flags(W, H, C.c_int32(flags), C.byref(bad)) == 1 and not bad.value


# ---- end to end -------------------------------------------------------------------------------------------------------------

def _device_loop(hpt, torch, scene, cams, W, H, seed, spp, guide_spp, depth, each_frame=None):
    """pt_cli --frames --reproject --guided --temporal-variance in Python, on one stream; each_frame(f, dict of device
    tensors, history) is called after frame f has finished.  Returns the last (filtered image, mean)."""
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    local = torch.zeros((hpt.local_pixels(W, H, hpt.make_params()), 3), dtype=torch.float32, device="cuda")
    frame, mean, alb, nrm, pos, var, out = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(7))
    cov, length, vout = (torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    with hpt.History(W, H, moments=True) as hist, hpt.Denoiser(W, H) as den:
        for f, cam in enumerate(cams):
            p = hpt.make_params(seed=seed, sample_offset=f * spp)
            moved = f == 0 or cam.tobytes() != cams[f - 1].tobytes()
            if moved:
                stream.synchronize()                             # the guide images are free: the last frame's filter has run
                scene.render_guides_device(cam, W, H, guide_spp, p, albedo=alb, normal=nrm, position=pos, coverage=cov)
                den.set_guides(alb, nrm, pos, cov, stream=st)
            scene.render_pt_device(cam, W, H, depth, spp, p, local.data_ptr(), st)
            hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, hpt.make_params(), st)
            hist.advance(cam, frame, *((nrm, pos, cov) if moved else (None, None, None)), mean_out=mean, stream=st)
            hist.length(length, stream=st)
            den.estimate_variance(frame, var, length, params=hpt.make_guided_params(demodulate=True), stream=st)
            if each_frame:
                stream.synchronize()
                estimate = var.cpu().numpy()
            hist.variance(var, fallback=var, stream=st)
            den.run_guided(mean, var, out, vout, params=hpt.make_guided_params(demodulate=True), stream=st)
            stream.synchronize()
            if each_frame:
                each_frame(f, dict(frame=frame, mean=mean, length=length, estimate=estimate, variance=var, out=out, v=vout), hist)
        return out.cpu().numpy(), mean.cpu().numpy()


def test_chain_on_the_device_equals_the_chain_of_the_oracles(hpt, torch, sio, oracle_mod, glib):
    """input.txt at 48 x 36, six frames of 2 spp: two from the scene's camera, then an orbit that grows by 0.5 degree per
    frame.  On the last frame the pixels that kept four frames or more are filtered under their own variance over time, the
    others under the spatial estimate."""
    sc, W, H, cams, k = chain_inputs(sio)
    L, sp, tr = sio.flatten_for_pt(sc)
    want = cpu_chain(sio, oracle_mod, glib)
    n_last = want[-1]["length"]
    assert (n_last >= 4).any() and (n_last < 4).any()                     # both branches of hpt_history_variance on the last frame
    assert want[-1]["variance"].tobytes() != want[-1]["estimate"].tobytes()

    def each_frame(f, d, hist):
        w = want[f]
        host = {key: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for key, v in d.items()}
        assert host["frame"].tobytes() == w["frame"].tobytes(), f
        assert host["length"].tobytes() == w["length"].tobytes(), f
        r = hist.read()
        assert r["mean"].tobytes() == w["mean"].tobytes() == host["mean"].tobytes() and r["q"].tobytes() == w["q"].tobytes(), f
        assert hist.metrics()["kept"] == w["kept"], f
        for key in ("estimate", "variance", "out", "v"):
            assert np.isfinite(w[key]).all(), (key, f)
            _same(host[key], w[key], (key, f))

    with hpt.Scene(L, sp, tr) as scene:
        _device_loop(hpt, torch, scene, cams, W, H, k["seed"], k["spp"], k["guide_spp"], k["depth"], each_frame)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(ROOT, "path_tracing_amd", "csrc", "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_temporal_variance_writes_the_image_of_the_python_chain(tmp_path, hpt, torch, sio):
    from test_host_mirror import _decode_png
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    W, H, frames = 48, 36, 6
    png, png_spatial = str(tmp_path / "out.png"), str(tmp_path / "spatial.png")
    base = ["--mode", "pt", "--input", scene_file, "--seed", 13, "--width", W, "--height", H, "--frames", frames, "--frame-spp", 2,
            "--orbit", 0.5, "--reproject", "--guided", "--guide-spp", 3]
    run = _cli(*base, "--temporal-variance", "--output", png)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    sc = sio.load_scene(scene_file)
    L, sp, tr = sio.flatten_for_pt(sc)
    cams = [sio.make_camera(hc.orbit_eye(sc.eye, sc.look_at, sc.view_up, f * 0.5), sc.look_at, sc.view_up, 50.0, W, H) for f in range(frames)]
    lengths = []
    with hpt.Scene(L, sp, tr) as scene:
        out, mean = _device_loop(hpt, torch, scene, cams, W, H, 13, 2, 3, 4, lambda f, d, hist: lengths.append(d["length"].cpu().numpy()))
    assert (lengths[-1] >= 4).any() and (lengths[-1] < 4).any()
    shown = _decode_png(open(png, "rb").read())
    assert np.array_equal(shown, hpt.tonemap(out))
    assert not np.array_equal(shown, hpt.tonemap(mean))
    run = _cli(*base, "--output", png_spatial)                           # without the flag: the spatial estimate everywhere
    assert run.returncode == 0, run.stdout + run.stderr
    assert not np.array_equal(_decode_png(open(png_spatial, "rb").read()), shown)
