"""The temporal history on the MI355X: hpt_history_* against the numpy oracle (tests/history_oracle.py) byte for byte and
integer for integer over the whole case table (tests/history_cases.py) -- no tolerance anywhere -- with every caller
image a view of one arena between sentinel bands; two histories on two streams; hpt_render_guides_device against
hpt_render_guides; the end-to-end chain against the chain of the oracles; and pt_cli --orbit / --reproject."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import history_cases as hc
import history_oracle as ho
from conftest import GOLDEN, ROOT
from test_history_cpu import chain_inputs, cpu_chain

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "path_tracing_amd", "csrc")
f32 = np.float32
SENTINEL = -7.25
BAND = 19          # floats between two images: no image starts on a 16-byte boundary by design


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def glib(tmp_path_factory):
    import guides_oracle
    return guides_oracle.build(tmp_path_factory.mktemp("guides_oracle"))


class Arena:
    """frame | normal | position | coverage | mean, BAND sentinels before, between and after, in one device tensor."""

    def __init__(self, torch, W, H):
        self.torch, self.n = torch, W * H
        sizes = [3 * self.n, 3 * self.n, 3 * self.n, self.n, 3 * self.n]
        self.off, at = [], BAND
        for s in sizes:
            self.off.append((at, s))
            at += s + BAND
        self.host = np.full(at, SENTINEL, f32)
        self.dev = torch.full((at,), SENTINEL, dtype=torch.float32, device="cuda")

    def view(self, k):
        lo, s = self.off[k]
        return self.dev[lo:lo + s]

    def load(self, frame, g):
        """The step's inputs into the arena; the mean image back to sentinels."""
        parts = [frame, g["normal"] if g else None, g["position"] if g else None, g["coverage"] if g else None, None]
        for k, a in enumerate(parts):
            lo, s = self.off[k]
            self.host[lo:lo + s] = SENTINEL if a is None else np.asarray(a, f32).reshape(-1)
        self.dev.copy_(self.torch.from_numpy(self.host))
        self.torch.cuda.synchronize()

    def check(self, mean, in_place):
        """Everything but the image the mean was written to is as it was loaded; returns nothing, asserts."""
        got = self.dev.cpu().numpy()
        want = self.host.copy()
        lo, s = self.off[0 if in_place else 4]
        want[lo:lo + s] = np.asarray(mean, f32).reshape(-1)
        assert got.tobytes() == want.tobytes(), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def _run_device(hpt, torch, steps, W, H, stream=0):
    """Per advance: (mean, length, kept, restarted, frames), as history_cases.run_oracle returns them."""
    arena = Arena(torch, W, H)
    out = []
    with hpt.History(W, H) as h:
        for step in steps:
            if step[0] == "reset":
                h.reset(stream=stream)
                continue
            a = step[1]
            g = a["guides"]
            arena.load(a["frame"], g)
            kw = dict(normal=arena.view(1), position=arena.view(2), coverage=arena.view(3)) if g else {}
            h.advance(a["camera"], arena.view(0), params=hpt.make_history_params(**a["params"]) if a["params"] else None,
                      mean_out=arena.view(0 if a["in_place"] else 4), stream=stream, **kw)
            m = h.metrics()
            r = h.read()
            arena.check(r["mean"], a["in_place"])              # mean-out holds the bytes read() returns, nothing else moved
            out.append((r["mean"], r["length"], m["kept"], m["restarted"], m["frames"]))
            assert r["frames"] == m["frames"]
    return out


def _assert_equal(got, want, name):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[2:] == w[2:], (name, k, g[2:], w[2:])
        bad = g[0].view(np.uint32) != w[0].view(np.uint32)
        assert not bad.any(), (name, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert g[1].tobytes() == w[1].tobytes(), (name, k)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_case_equals_the_oracle(hpt, torch, name):
    steps = hc.CASES[name]
    W, H = hc.size_of(steps)
    _assert_equal(_run_device(hpt, torch, steps, W, H), hc.run_oracle(steps, W, H), name)


def test_two_histories_of_different_sizes_on_two_streams(hpt, torch):
    names = ("size_67x3", "orbit_5")
    steps = [hc.CASES[n] for n in names]
    sizes = [hc.size_of(s) for s in steps]
    want = [hc.run_oracle(s, *wh) for s, wh in zip(steps, sizes)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams[0].cuda_stream != streams[1].cuda_stream != 0
    hist = [hpt.History(*wh) for wh in sizes]
    dev = [[{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(s[1]["guides"], frame=s[1]["frame"]).items()} for s in st] for st in steps]
    means = [[torch.full((wh[1], wh[0], 3), SENTINEL, dtype=torch.float32, device="cuda") for _ in st] for st, wh in zip(steps, sizes)]
    torch.cuda.synchronize()
    try:
        counts = [[], []]
        for k in range(max(len(s) for s in steps)):
            for i in (0, 1):
                if k < len(steps[i]):
                    d = dev[i][k]
                    hist[i].advance(steps[i][k][1]["camera"], d["frame"], d["normal"], d["position"], d["coverage"], mean_out=means[i][k],
                                    stream=streams[i].cuda_stream)
            for i in (0, 1):
                if k < len(steps[i]):
                    m = hist[i].metrics()
                    counts[i].append((m["kept"], m["restarted"], m["frames"]))
        for i in (0, 1):
            streams[i].synchronize()
            assert counts[i] == [w[2:] for w in want[i]], names[i]
            for k, w in enumerate(want[i]):
                assert means[i][k].cpu().numpy().tobytes() == w[0].tobytes(), (names[i], k)
            r = hist[i].read()
            assert r["mean"].tobytes() == want[i][-1][0].tobytes() and r["length"].tobytes() == want[i][-1][1].tobytes()
    finally:
        for h in hist:
            h.close()


def test_refusals_on_a_live_object_enqueue_nothing(hpt, torch):
    lib = hpt.load_library()
    W, H = 5, 3
    cam = hc.camera(W, H)
    buf = torch.full((8 * W * H * 3,), SENTINEL, dtype=torch.float32, device="cuda")
    n = W * H * 3
    frame, nrm, pos, cov, out = buf[:n], buf[n:2 * n], buf[2 * n:3 * n], buf[3 * n:3 * n + W * H], buf[4 * n:5 * n]
    with hpt.History(W, H) as h:
        with pytest.raises(hpt.HptError, match="hpt error 1:.*before the first"):
            h.metrics()
        bad = hpt.make_history_params(max_history=0.25)
        flat = np.array(cam)
        flat["dy"] = flat["dx"]
        for kw, word in ((dict(normal=nrm), "all three"), (dict(normal=nrm, position=pos), "all three"), (dict(params=bad), "max_history"),
                         (dict(mean_out=buf[1:1 + n]), "overlap"), (dict(normal=nrm, position=pos, coverage=buf[3 * n - 1:]), "overlap"),
                         (dict(camera=flat), "degenerate")):
            args = dict(camera=cam, frame=frame, mean_out=out)
            args.update(kw)
            with pytest.raises(hpt.HptError, match="hpt error 1:.*" + word):
                h.advance(args.pop("camera"), args.pop("frame"), **args)
        camv = np.ascontiguousarray(cam, hpt.CAMERA).reshape(1).ctypes.data_as(C.c_void_p)
        assert lib.hpt_history_advance(h._h, camv, None, None, None, None, None, None, None) == 1 and b"null frame" in lib.hpt_last_error()
        assert lib.hpt_history_advance(h._h, None, C.c_void_p(frame.data_ptr()), None, None, None, None, None, None) == 1
        with pytest.raises(hpt.HptError):
            h.metrics()                                                 # nothing was advanced by the refused calls
        r = h.read()
        assert r["frames"] == 0 and not r["mean"].any() and not r["length"].any()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == f32(SENTINEL)).all()
        h.advance(cam, frame, mean_out=frame)                           # guides are optional from the first frame on
        assert h.metrics() == dict(kept=0, restarted=0, frames=1)
        h.reset()
        with pytest.raises(hpt.HptError):
            h.metrics()
        assert h.read()["frames"] == 0 and not h.read()["length"].any()


# ---- guides that stay on the device ----------------------------------------------------------------------------------------

KEYS = ("albedo", "normal", "position", "coverage")


def _device_guides(hpt, torch, scene, cam, W, H, spp, p, which=KEYS):
    bufs = {k: torch.full((H, W) if k == "coverage" else (H, W, 3), SENTINEL, dtype=torch.float32, device="cuda") for k in KEYS}
    torch.cuda.synchronize()
    scene.render_guides_device(cam, W, H, spp, p, **{k: bufs[k] for k in which})
    return {k: v.cpu().numpy() for k, v in bufs.items()}        # no synchronise: the call returns when they are complete


@pytest.mark.parametrize("size", [(50, 37), (1, 1), (40, 1)])
def test_render_guides_device_gives_the_bytes_of_render_guides(hpt, torch, sio, input_scene, size):
    W, H = size
    sc, (L, sp, tr) = input_scene
    cam = sio.camera_for(sc, W, H)
    p = hpt.make_params(seed=11, sample_offset=3)
    with hpt.Scene(L, sp, tr) as s:
        host = s.render_guides(cam, W, H, 3, p)
        dev = _device_guides(hpt, torch, s, cam, W, H, 3, p)
        assert host["coverage"].max() == 3
        for k in KEYS:
            assert dev[k].tobytes() == host[k].tobytes(), k
        for only in KEYS:                                        # any may be NULL; the others are left alone
            one = _device_guides(hpt, torch, s, cam, W, H, 3, p, which=(only,))
            for k in KEYS:
                assert one[k].tobytes() == (host[k].tobytes() if k == only else np.full_like(host[k], SENTINEL).tobytes()), (only, k)
        with pytest.raises(hpt.HptError, match="hpt error 1:.*every output is null"):
            s.render_guides_device(cam, W, H, 3, p)
        with pytest.raises(hpt.HptError, match="hpt error 1:"):
            s.render_guides_device(cam, W, H, 0, p, coverage=0x1000)
        assert s.render_guides(cam, W, H, 3, p)["normal"].tobytes() == host["normal"].tobytes()      # the host call is as it was


# ---- end to end --------------------------------------------------------------------------------------------------------------

def _device_chain(hpt, torch, scene, cams, W, H, seed, spp, guide_spp, depth):
    """render_guides_device (frame 0 and moved frames), render_pt_device, untile, History.advance, Display.present on one
    stream: per frame (frame, mean, bytes, kept)."""
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    local = torch.zeros((hpt.local_pixels(W, H, hpt.make_params()), 3), dtype=torch.float32, device="cuda")
    frame, mean, nrm, pos = (torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(4))
    cov = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = []
    with hpt.History(W, H) as hist, hpt.Display(W, H) as disp:
        for f, cam in enumerate(cams):
            p = hpt.make_params(seed=seed, sample_offset=f * spp)
            guides = f == 0 or np.asarray(cam).tobytes() != np.asarray(cams[f - 1]).tobytes()
            if guides:                                           # blocking, before this frame's work is enqueued on `st`
                scene.render_guides_device(cam, W, H, guide_spp, p, normal=nrm, position=pos, coverage=cov)
            scene.render_pt_device(cam, W, H, depth, spp, p, local.data_ptr(), st)
            hpt.untile(local.data_ptr(), frame.data_ptr(), W, H, hpt.make_params(), st)
            hist.advance(cam, frame, *((nrm, pos, cov) if guides else (None, None, None)), mean_out=mean, stream=st)
            disp.present(mean, out=rgb8, stream=st)
            kept = hist.metrics()["kept"]
            stream.synchronize()
            out.append((frame.cpu().numpy(), mean.cpu().numpy(), rgb8.cpu().numpy(), kept))
    return out


def test_end_to_end_chain_on_the_device_equals_the_chain_of_the_oracles(hpt, torch, sio, oracle_mod, glib):
    sc, W, H, cams, k = chain_inputs(sio)
    L, sp, tr = sio.flatten_for_pt(sc)
    want = cpu_chain(sio, oracle_mod, glib)
    with hpt.Scene(L, sp, tr) as scene:
        got = _device_chain(hpt, torch, scene, cams, W, H, k["seed"], k["spp"], k["guide_spp"], k["depth"])
    for f, ((w_frame, _, w_mean, w_kept), (g_frame, g_mean, _, g_kept)) in enumerate(zip(want, got)):
        assert g_frame.tobytes() == w_frame.tobytes(), f
        assert g_mean.tobytes() == w_mean.tobytes(), f
        assert g_kept == w_kept, f
    assert 0 < got[-1][3] < W * H


# ---- CLI ---------------------------------------------------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([os.path.join(CSRC, "pt_cli")] + [str(a) for a in args], capture_output=True, text=True)


def _orbit_cameras(sio, sc, W, H, frames, degrees):
    return [sio.make_camera(hc.orbit_eye(sc.eye, sc.look_at, sc.view_up, f * degrees), sc.look_at, sc.view_up, 50.0, W, H) for f in range(frames)]


def test_cli_orbit_reproject_writes_the_image_of_the_python_chain(tmp_path, hpt, torch, sio):
    from test_host_mirror import _decode_png
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    W, H = 64, 48
    png = str(tmp_path / "out.png")
    run = _cli("--mode", "pt", "--input", scene_file, "--seed", 13, "--width", W, "--height", H, "--frames", 4, "--frame-spp", 2,
               "--orbit", 2, "--reproject", "--guide-spp", 3, "--output", png)
    assert run.returncode == 0 and "[Success] Image saved!" in run.stdout, run.stdout + run.stderr
    sc = sio.load_scene(scene_file)
    L, sp, tr = sio.flatten_for_pt(sc)
    cams = _orbit_cameras(sio, sc, W, H, 4, 2.0)
    assert len({c.tobytes() for c in cams}) == 4
    with hpt.Scene(L, sp, tr) as scene:
        chain = _device_chain(hpt, torch, scene, cams, W, H, 13, 2, 3, 4)
    assert np.array_equal(_decode_png(open(png, "rb").read()), chain[-1][2])
    lines = re.findall(r"^\[Frame (\d+)\] rms (\S+) kept (\S+) %$", run.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == [1, 2, 3, 4]
    assert [l[2] for l in lines] == ["%.1f" % (100.0 * c[3] / (W * H)) for c in chain]
    assert chain[0][3] == 0 and all(0 < c[3] < W * H for c in chain[1:])
    assert chain[-1][1].tobytes() != chain[-1][0].tobytes()             # the last mean is not the last frame alone


def test_cli_orbit_alone_restarts_and_no_flag_is_the_loop_as_it_was(tmp_path, hpt, torch, sio):
    from test_host_mirror import _decode_png
    scene_file = os.path.join(GOLDEN, "scenes", "input.txt")
    W, H = 40, 32
    png = str(tmp_path / "out.png")
    base = ["--mode", "pt", "--input", scene_file, "--seed", 13, "--width", W, "--height", H, "--frames", 3, "--frame-spp", 2, "--output", png]
    sc = sio.load_scene(scene_file)
    L, sp, tr = sio.flatten_for_pt(sc)
    cams = _orbit_cameras(sio, sc, W, H, 3, 2.0)
    with hpt.Scene(L, sp, tr) as scene:
        moved_last = scene.render_pt(cams[2], W, H, 4, 2, hpt.make_params(seed=13, sample_offset=4))
        still = [scene.render_pt(sio.camera_for(sc, W, H, 50.0), W, H, 4, 2, hpt.make_params(seed=13, sample_offset=2 * f)) for f in range(3)]
    # --orbit alone: every moved frame resets the accumulator, so the picture is the last frame's
    run = _cli(*base, "--orbit", 2)
    assert run.returncode == 0, run.stdout + run.stderr
    assert np.array_equal(_decode_png(open(png, "rb").read()), hpt.tonemap(moved_last))
    assert "kept" not in run.stdout
    # no flag: the accumulated mean of the three frames, and frame lines without a share
    run = _cli(*base)
    assert run.returncode == 0, run.stdout + run.stderr
    mean = ((still[0] + still[1]) + still[2]) / f32(3)
    assert np.array_equal(_decode_png(open(png, "rb").read()), hpt.tonemap(mean))
    assert len(re.findall(r"^\[Frame \d+\] rms \S+$", run.stdout, flags=re.M)) == 3 and "kept" not in run.stdout
    # --reproject with a still camera is the same running mean (identity: no test applied)
    run = _cli(*base, "--reproject")
    assert run.returncode == 0, run.stdout + run.stderr
    lines = re.findall(r"^\[Frame \d+\] rms \S+ kept (\S+) %$", run.stdout, flags=re.M)
    assert lines == ["0.0", "100.0", "100.0"]
    m = (still[0] * f32(1) + still[1]) / f32(2)
    m = (m * f32(2) + still[2]) / f32(3)
    assert np.array_equal(_decode_png(open(png, "rb").read()), hpt.tonemap(m))
    for flags in (["--orbit", 2], ["--reproject"]):
        run = _cli("--mode", "pt", "--input", scene_file, "--output", tmp_path / "x.png", *flags)
        assert run.returncode != 0 and "need --frames" in run.stderr
    assert not os.path.exists(tmp_path / "x.png")
