"""ctypes bindings for tests/emu/libapemu_rhythm.so (TEST INFRASTRUCTURE ONLY).

Runs the rhythm kernel source (kernels_rhythm.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_rhythm.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float

BAND = 64          # NaN floats (0xFF bytes for the masks) before and after every buffer


def build(force=False):
    srcs = [os.path.join(HERE, "emu_rhythm.cpp"), os.path.join(CSRC, "host_builders.cpp")]
    deps = srcs + [os.path.join(HERE, "emu_shim.h"), os.path.join(ROOT, "include", "audioprims.h")] + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")
    ]
    if not force and os.path.exists(LIB):
        if os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
            return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", tmp] + srcs)
    os.replace(tmp, LIB)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.emu_rhythm_last_error.restype = ctypes.c_char_p
        _lib.emu_tempogram_agg_floats.argtypes = [_i64, _i64, _int, _int]
        _lib.emu_tempogram_agg_floats.restype = _i64
        _lib.emu_beat_half.argtypes = [_int]
        _lib.ap_twiddle_table_host.argtypes = [_int, _p]
        _lib.emu_tempogram_f32.argtypes = [_p, _i64, _i64, _i64, _p, _int, _int, _int, _p, _p, _p, _int]
        _lib.emu_tempo_pick_f32.argtypes = [_p, _i64, _i64, _int, _i64, _i64, _i64, _i64, _i64, _f, _p, _p, _int]
        _lib.emu_beat_track_f32.argtypes = [_p, _i64, _i64, _i64, _p, _f, _int, _p, _p, _p, _p, _p, _int]
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_rhythm_last_error().decode())


def last_error():
    return lib().emu_rhythm_last_error().decode()


def lds_overruns():
    return int(lib().emu_rhythm_lds_overruns())


def max_frames():
    return int(lib().emu_beat_track_max_frames())


def max_period():
    return int(lib().emu_beat_track_max_period())


def max_win():
    return int(lib().emu_tempogram_max_win())


def half(P):
    return int(lib().emu_beat_half(P))


class _Guarded:
    """A (..., rs) buffer between two bands of a fill value (NaN for floats), its pad columns T .. rs - 1 filled too."""

    def __init__(self, lead, T, rs, data=None, dtype=np.float32, fill=np.nan):
        self.shape, self.T, self.fill = tuple(lead) + (rs,), T, fill
        n = int(np.prod(self.shape))
        self.raw = np.full(n + 2 * BAND, fill, dtype)
        self.body = self.raw[BAND:BAND + n].reshape(self.shape)
        if data is not None:
            self.body[..., :T] = data
        self.ptr = self.raw.ctypes.data + self.raw.itemsize * BAND

    def _is_fill(self, a):
        return np.isnan(a) if isinstance(self.fill, float) and np.isnan(self.fill) else a == self.fill

    def intact(self, written):
        """The bands and the pad columns still hold the fill value; `written`: the payload holds it nowhere any more."""
        ok = self._is_fill(self.raw[:BAND]).all() and self._is_fill(self.raw[-BAND:]).all() and self._is_fill(self.body[..., self.T:]).all()
        return bool(ok and (not written or not self._is_fill(self.body[..., :self.T]).any()))


WAVE_WMAX = 512


def twiddles(n=1024):
    tw = np.empty(2 * n, np.float32)
    _check(lib().ap_twiddle_table_host(n, tw.ctypes.data))
    return tw


def tempogram(e, window, *, center=True, norm=True, pad_in=0, out=True, agg=False, grid=0, wave=False):
    """(tg (B, W, T) or None, tile sums (B, n_tiles, W) or None) of a (B, n) float32 envelope through the emulated C
    entry; wave: the wave-per-frame kernel (win_length <= 512), else the general one.  The envelope lies between NaN bands with pad_in NaN columns per row, the outputs between NaN bands: asserted
    unwritten, and no NaN comes out (a read of a band or a pad column would put one there)."""
    e = np.asarray(e, np.float32)
    w = np.ascontiguousarray(window, np.float32)
    B, n = e.shape
    W = len(w)
    T = n if center else n - W + 1
    src = _Guarded((B,), n, n + pad_in, e)
    wsrc = _Guarded((), W, W, w)
    o = _Guarded((B, W), T, T) if out else None
    n_agg = int(lib().emu_tempogram_agg_floats(B, n, W, int(center)))
    a = _Guarded((), n_agg, n_agg) if agg else None
    tw = twiddles() if wave else None
    _check(lib().emu_tempogram_f32(src.ptr, B, n, n + pad_in, wsrc.ptr, W, int(center), int(norm),
                                   None if tw is None else tw.ctypes.data, None if o is None else o.ptr,
                                   None if a is None else a.ptr, grid))
    assert src.intact(written=False) and wsrc.intact(written=False)
    assert o is None or o.intact(written=True), "a band was written, or a value is NaN"
    assert a is None or a.intact(written=True), "a band was written, or a value is NaN"
    return (None if o is None else o.body.copy(), None if a is None else a.body.reshape(B, -1, W).copy())


def tempogram_raw(e_ptr, B, n, rs, w_ptr, W, center, out_ptr, agg_ptr, tw_ptr=None):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_tempogram_f32(e_ptr, B, n, rs, w_ptr, W, center, 1, tw_ptr, out_ptr, agg_ptr, 0)


def tempo_pick(g, prior, *, n_col, sb, sk, sc, n_red, sr, div, grid=0):
    """(B, n_col) int32 picks from the float32 array g (B leading) with the strides of ap_tempo_pick_f32."""
    g = np.ascontiguousarray(g, np.float32)
    prior = np.ascontiguousarray(prior, np.float32)
    B, W = g.shape[0], len(prior)
    src = _Guarded((), g.size, g.size, g.reshape(-1))
    psrc = _Guarded((), W, W, prior)
    idx = _Guarded((), B * n_col, B * n_col, dtype=np.int32, fill=-7)
    _check(lib().emu_tempo_pick_f32(src.ptr, B, n_col, W, sb, sk, sc, n_red, sr, float(div), psrc.ptr, idx.ptr, grid))
    assert idx.intact(written=True)
    return idx.body.reshape(B, n_col).copy()


def beat_track(x, period, *, tightness=100.0, trim=True, pad_in=0, stages=False, grid=0):
    """(mask (B, T) bool, count (B,)) or, with stages, (mask, count, L, C, link) of a (B, T) float32 array (NaN allowed)
    and (B,) periods through the emulated C entry; every buffer between guard bands."""
    x = np.asarray(x, np.float32)
    B, T = x.shape
    src = _Guarded((B,), T, T + pad_in, x)
    per = _Guarded((), B, B, np.asarray(period, np.int32), dtype=np.int32, fill=-7)
    mask = _Guarded((), B * T, B * T, dtype=np.uint8, fill=0xFF)
    cnt = _Guarded((), B, B, dtype=np.int32, fill=-7)
    L = _Guarded((B,), T, T) if stages else None
    C = _Guarded((B,), T, T) if stages else None
    link = _Guarded((B,), T, T, dtype=np.int32, fill=-2 ** 31) if stages else None       # (a link may be any i - d >= -2P)
    _check(lib().emu_beat_track_f32(src.ptr, B, T, T + pad_in, per.ptr, float(tightness), int(trim), mask.ptr, cnt.ptr,
                                    None if L is None else L.ptr, None if C is None else C.ptr,
                                    None if link is None else link.ptr, grid))
    assert mask.intact(written=True) and cnt.intact(written=True), "a band was written"
    assert np.isnan(src.raw[:BAND]).all() and np.isnan(src.raw[-BAND:]).all() and np.isnan(src.body[:, T:]).all()
    m = mask.body.reshape(B, T)
    assert set(np.unique(m)) <= {0, 1}
    c = cnt.body.copy()
    assert np.array_equal(m.sum(axis=1), np.maximum(c, 0))
    if not stages:
        return m.astype(bool), c
    assert L.intact(written=False) and C.intact(written=False) and link.intact(written=True)
    return m.astype(bool), c, L.body.copy(), C.body.copy(), link.body.copy()


def beat_track_raw(x_ptr, B, T, rs, period_ptr, tightness, mask_ptr, count_ptr):
    return lib().emu_beat_track_f32(x_ptr, B, T, rs, period_ptr, tightness, 1, mask_ptr, count_ptr, None, None, None, 0)
