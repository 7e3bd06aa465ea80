"""numpy restatement of the progressive display (include/hpt.h, "progressive display"): everything except the byte function.
Float32 adds in frame order, the division, the variance expression, flip, pitch, offset, BGR and uint64 sums of squared
byte differences are written out here; the bytes come from hpt_tonemap_reference, the host loop that
tests/test_host_mirror.py holds the device tone map to (it needs libhpt.so, not a device)."""
import ctypes as C

import numpy as np

f32 = np.float32


def _lib():
    import path_tracing_amd
    return path_tracing_amd.load_library()


def thresholds():
    """hpt_tonemap_table: [k] = the smallest float whose byte is >= k, [0] = -inf."""
    thr = np.zeros(256, f32)
    lib = _lib()
    lib.hpt_tonemap_table.restype = None
    lib.hpt_tonemap_table(thr.ctypes.data_as(C.c_void_p))
    return thr


def tone_bytes(linear):
    """The canonical bytes b[r][x][c] of a float32 [H, W, 3] image (RGB, row 0 = top)."""
    img = np.ascontiguousarray(linear, f32)
    out = np.zeros(img.shape, np.uint8)
    lib = _lib()
    lib.hpt_tonemap_reference.restype = None
    lib.hpt_tonemap_reference(img.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_int64(img.size // 3), 0)
    return out


class Accum:
    """hpt_accum: sum = sum + v, sq = sq + v * v, each operation rounded to float32 (numpy float32 arrays do exactly that)."""

    def __init__(self, W, H, moments=False):
        self.shape = (H, W, 3)
        self.moments = moments
        self.reset()

    def reset(self):
        self.sum = np.zeros(self.shape, f32)
        self.sq = np.zeros(self.shape, f32) if self.moments else None
        self.count = 0

    def add(self, frame):
        """Returns the mean that d_mean_out receives."""
        v = np.asarray(frame, f32).reshape(self.shape)
        with np.errstate(all="ignore"):
            self.sum = self.sum + v
            if self.moments:
                self.sq = self.sq + v * v
        self.count += 1
        return self.mean()

    def mean(self):
        assert self.count > 0
        with np.errstate(all="ignore"):
            return self.sum / f32(self.count)

    def variance(self):
        assert self.moments
        if self.count < 2:
            return np.zeros(self.shape, f32)
        with np.errstate(all="ignore"):
            k = f32(self.count)
            m = self.sum / k
            q = self.sq / k
            d = q - m * m
            return np.fmax(d, f32(0.0)) / f32(self.count - 1)       # fmaxf: a NaN difference gives 0


def ssd(a, b):
    """Sum of squared byte differences as an exact Python int (uint64 on the device)."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def rms(s):
    return float(np.sqrt(np.float64(s)) / 255.0)


class Display:
    """hpt_display: `last` in canonical order, P presents so far."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.last = None
        self.presented = 0

    def reset(self):
        self.last = None
        self.presented = 0

    def present(self, linear, other=None, out=None, pitch=0, x_offset=0, bgr=False, flip_y=False):
        """out: a flat uint8 array standing for d_rgb8 (written in place).  Returns (ssd_prev, ssd_other)."""
        W, H = self.W, self.H
        b = tone_bytes(np.asarray(linear, f32).reshape(H, W, 3))
        s_prev = ssd(b, self.last) if self.presented > 0 else 0
        s_other = 0
        if other is not None:
            assert other is not self and other.presented > 0 and (other.W, other.H) == (W, H)
            s_other = ssd(b, other.last)
        if out is not None:
            pitch = pitch or 3 * W
            assert x_offset >= 0 and pitch >= x_offset + 3 * W
            for r in range(H):
                row = b[r, :, ::-1] if bgr else b[r]
                at = (H - 1 - r if flip_y else r) * pitch + x_offset
                out[at: at + 3 * W] = row.reshape(-1)
        self.last = b
        self.presented += 1
        return s_prev, s_other


def reference_rms(current, last):
    """Literal transcription of the reference's RMS, src/main.cpp:421-425, 502-509, 521: a float running sum of
    powf(diff, 2) over columns (outer), rows (inner) and channels, then sqrt(.) / 255.0f in float.  The row flip of
    main.cpp:431 moves both operands alike.  Returns (the float sum, the float rms)."""
    H, W = current.shape[:2]
    cur = current.astype(np.int32)
    lst = last.astype(np.int32)
    acc = f32(0.0)
    for i in range(W):
        for j in range(H):
            for k in range(3):
                d = f32(int(cur[j, i, k]) - int(lst[j, i, k]))
                acc = f32(acc + f32(d * d))                       # powf(d, 2) of an integer |d| <= 255 is exact
    return acc, f32(np.sqrt(acc) / f32(255.0))
