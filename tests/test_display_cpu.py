"""CPU tests of the progressive display (include/hpt.h, "progressive display"): the numpy oracle against a literal
transcription of the reference's RMS loop, the sanity of the case table the device is held to, the refusals the host makes
before it touches a device, and the presence of the calls in the header and of the Python classes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_cases as dc
import display_oracle as do
from conftest import ROOT

HPT_ERR_INVALID = 1
f32 = np.float32


@pytest.fixture(scope="module")
def expected():
    return {c["name"]: dc.expected(c) for c in dc.CASES}


# ---- the oracle against the reference's loop ----------------------------------------------------------------------------

def test_rms_equals_the_reference_loop_up_to_2_pow_24(expected):
    """While the sum of squares stays at or below 2^24 every partial sum of the reference's float accumulator is an exact
    integer, so its sum IS the integer sum; its rms then differs from sqrt((double) ssd) / 255.0 by float rounding of the
    square root and of the quotient only (two roundings, each 2^-24 relative)."""
    checked = 0
    for c in dc.CASES:
        exp = expected[c["name"]]
        if c["W"] * c["H"] * 3 > 6000:
            continue                                    # the transcription is a Python loop
        for (b, s_prev), (last, _) in zip(exp[1:], exp[:-1]):
            if s_prev > 2 ** 24:
                continue
            acc, r = do.reference_rms(b, last)
            assert float(acc) == float(s_prev) and int(acc) == s_prev
            assert r == f32(np.sqrt(f32(s_prev)) / f32(255.0))
            assert abs(float(r) - do.rms(s_prev)) <= 2.0 ** -23 * (1.0 + 2.0 ** -20) * do.rms(s_prev)   # + their product and the double's own
            checked += 1
    assert checked >= 8


def test_reference_float_sum_parts_from_the_integer_above_2_pow_24(expected):
    """10 x 10, black then white: 300 terms of 65025 = 19 507 500 > 2^24.  From the 259th term on the float accumulator
    holds even numbers only and every add of the odd 65025 rounds; the integer sum is the number it approximates."""
    (black, _), (white, s_prev) = expected["black_white_10x10"]
    assert s_prev == 300 * 65025 > 2 ** 24
    acc, r = do.reference_rms(white, black)
    assert float(acc) != float(s_prev)
    assert abs(float(acc) - s_prev) <= 42               # terms 259 .. 300: 42 adds, each rounded by at most half a unit of 2
    assert abs(float(r) - do.rms(s_prev)) <= (21.0 / s_prev + 2.0 ** -22) * do.rms(s_prev)


def test_accum_oracle_is_float32_in_frame_order():
    a = do.Accum(1, 1, moments=True)
    m = a.add(np.array([[[0.1, -2.0, 3.0]]], f32))
    assert m.dtype == f32 and m.tobytes() == (np.array([[[0.1, -2.0, 3.0]]], f32) / f32(1)).tobytes()
    assert a.variance().tobytes() == np.zeros((1, 1, 3), f32).tobytes()          # K < 2
    a.add(np.array([[[0.3, -2.0, 1e8]]], f32))
    a.add(np.array([[[1.0, -2.0, 1.0]]], f32))
    assert a.sum[0, 0, 2] == f32(f32(f32(3.0) + f32(1e8)) + f32(1.0)) == f32(1e8)   # 1e8 swallows the small terms: order shows
    assert a.variance()[0, 0, 1] == 0.0 and a.variance()[0, 0, 0] > 0.0
    assert a.mean()[0, 0, 0] == f32(f32(f32(0.1) + f32(0.3)) + f32(1.0)) / f32(3)


def test_display_oracle_layout():
    """flip, pitch, offset and BGR of one 2 x 2 image written into the middle panel of a three-panel framebuffer."""
    W = H = 2
    img = np.array([[[0.0, 0.25, 1.0], [0.5, 0.5, 0.5]], [[1.0, 0.0, 0.0], [0.1, 0.2, 0.3]]], f32)
    b = do.tone_bytes(img)
    assert b[0, 0].tolist() == [0, 135, 255]
    fb = np.full(H * 9 * W, dc.SENTINEL, np.uint8)
    d = do.Display(W, H)
    assert d.present(img, out=fb, pitch=9 * W, x_offset=3 * W, bgr=True, flip_y=True) == (0, 0)
    rows = fb.reshape(H, 9 * W)
    assert (rows[:, :6] == dc.SENTINEL).all() and (rows[:, 12:] == dc.SENTINEL).all()
    assert rows[1, 6:12].tolist() == b[0, :, ::-1].reshape(-1).tolist()            # image row 0 at the bottom, B G R
    assert rows[0, 6:12].tolist() == b[1, :, ::-1].reshape(-1).tolist()
    assert d.last.tobytes() == b.tobytes()                                          # canonical whatever the flags
    s_prev, _ = d.present(img[::-1].copy())
    assert s_prev == do.ssd(b, b[::-1]) > 0


# ---- the case table -----------------------------------------------------------------------------------------------------

def test_case_table_is_sane(expected):
    assert [(c["W"], c["H"]) for c in dc.CASES[:7]] == [(1, 1), (3, 2), (50, 37), (64, 4), (65, 5), (256, 1), (130, 67)]
    for c in dc.CASES:
        frames = c["frames"]()
        exp = expected[c["name"]]
        assert len(frames) >= 2 and exp[0][1] == 0
        if not c["repeat"]:
            for i in range(len(frames)):
                for j in range(i):
                    assert frames[i].tobytes() != frames[j].tobytes(), (c["name"], i, j)
            assert all(s > 0 for _, s in exp[1:]), c["name"]
        else:
            assert any(s == 0 for _, s in exp[1:]) and any(s > 0 for _, s in exp[1:])
        for b, _ in exp:
            if not c["flat"]:
                assert not (b == 0).all() and not (b == 255).all(), c["name"]
    assert expected["black_white_256x96"][1][1] == dc.BLACK_WHITE_SSD > 2 ** 32


def test_special_values_hit_both_sides_of_their_thresholds():
    sp = dc.special_values()
    b = do.tone_bytes(np.resize(sp, (1, (len(sp) + 2) // 3, 3)))[0].reshape(-1)[: len(sp)]
    assert b[:5].tolist() == [0, 255, 0, 0, 255] and b[6:9].tolist() == [255, 0, 255]     # NaN, inf, -inf, -0, 1 | 1+, -tiny, huge
    assert b[9:].tolist() == [1, 0, 2, 1, 127, 126, 128, 127, 200, 199, 255, 254]         # a threshold and the float below it
    frames = dc.present_frames(50, 37)
    assert np.isnan(frames[0]).any() and np.isinf(frames[1]).any() and np.isfinite(frames[2]).all()


def test_accum_frames_cover_zero_negative_and_large():
    for W, H in dc.ACCUM_SIZES:
        frames = dc.accum_frames(W, H, 17)
        assert len({f.tobytes() for f in frames}) == 17
        allv = np.concatenate([f.reshape(-1) for f in frames])
        assert (allv == 0).any() and (allv < 0).any() and (allv > 1).any()


# ---- the boundary -------------------------------------------------------------------------------------------------------

DECLARED = ["hpt_accum_create", "hpt_accum_add", "hpt_accum_mean", "hpt_accum_variance", "hpt_accum_reset", "hpt_accum_count",
            "hpt_accum_read", "hpt_accum_destroy", "hpt_display_create", "hpt_display_present", "hpt_display_metrics",
            "hpt_display_reset", "hpt_display_destroy"]


def test_header_declares_the_calls_and_python_has_the_classes(hpt):
    text = open(os.path.join(ROOT, "include", "hpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = hpt.load_library()
    for name in DECLARED:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    for macro, value in (("HPT_ACCUM_MOMENTS", 1), ("HPT_DISPLAY_BGR", 1), ("HPT_DISPLAY_FLIP_Y", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    assert "2^24" in text and "1e-7" in text            # the header says where the variance and the reference's sum stop
    for cls, methods in ((hpt.Accumulator, ("add", "mean", "variance", "reset", "count", "read", "close", "__enter__", "__exit__")),
                         (hpt.Display, ("present", "metrics", "reset", "close", "__enter__", "__exit__"))):
        for m in methods:
            assert hasattr(cls, m), (cls, m)
    assert (hpt.ACCUM_MOMENTS, hpt.DISPLAY_BGR, hpt.DISPLAY_FLIP_Y) == (1, 1, 2)


def _refused(lib, rc, *words):
    assert rc == HPT_ERR_INVALID, (rc, lib.hpt_last_error())
    msg = lib.hpt_last_error()
    assert msg and all(w in msg for w in words), msg


def test_refusals_before_the_device_is_touched(hpt):
    """No device is needed (and none is there under -m "not gpu"): every check below comes before the first HIP call.
    The refusals that need a live object -- variance without MOMENTS, a NULL frame, an overlap, a bad pitch, `other` --
    are in tests/test_gpu_display.py."""
    lib = hpt.load_library()
    h = C.c_void_p()
    for W, H in ((0, 4), (4, 0), (-1, 4), (4, -7)):
        _refused(lib, lib.hpt_accum_create(W, H, 0, C.byref(h)), b"positive")
        assert not h.value
        _refused(lib, lib.hpt_display_create(W, H, C.byref(h)), b"positive")
        assert not h.value
    _refused(lib, lib.hpt_accum_create(1 << 15, 1 << 14, 0, C.byref(h)), b"too large")
    for flags in (2, 3, 1 << 30, -2):
        _refused(lib, lib.hpt_accum_create(4, 4, C.c_int32(flags), C.byref(h)), b"HPT_ACCUM_MOMENTS")
    _refused(lib, lib.hpt_accum_create(4, 4, 0, None), b"null")
    _refused(lib, lib.hpt_display_create(4, 4, None), b"null")
    buf = (C.c_float * 16)()
    _refused(lib, lib.hpt_accum_add(None, buf, None, None), b"null accumulator")
    _refused(lib, lib.hpt_accum_mean(None, buf, None), b"null accumulator")
    _refused(lib, lib.hpt_accum_variance(None, buf, None), b"null accumulator")
    _refused(lib, lib.hpt_accum_reset(None, None), b"null accumulator")
    _refused(lib, lib.hpt_accum_read(None, None, None, None), b"null accumulator")
    assert lib.hpt_accum_count(None) == 0
    _refused(lib, lib.hpt_display_present(None, buf, None, None, C.c_int64(0), C.c_int64(0), 0, None), b"null display")
    _refused(lib, lib.hpt_display_metrics(None, None, None, None, None, None), b"null display")
    _refused(lib, lib.hpt_display_reset(None, None), b"null display")
    lib.hpt_accum_destroy(None)
    lib.hpt_display_destroy(None)
