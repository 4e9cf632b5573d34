"""ctypes bindings for tests/emu/libapemu_onset.so (TEST INFRASTRUCTURE ONLY).

Runs the onset kernel source (kernels_onset.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_onset.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float

BAND = 64          # NaN floats (0xFF bytes for the masks) before and after every buffer


def build(force=False):
    srcs = [os.path.join(HERE, "emu_onset.cpp")]
    deps = srcs + [os.path.join(HERE, "emu_shim.h"), os.path.join(ROOT, "include", "audioprims.h")] + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")
    ]
    if not force and os.path.exists(LIB):
        if os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
            return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-o", tmp] + srcs)
    os.replace(tmp, LIB)
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.emu_onset_last_error.restype = ctypes.c_char_p
        _lib.emu_onset_geometry.restype = ctypes.POINTER(ctypes.c_int)
        _lib.emu_onset_fkey.argtypes = [_f]
        _lib.emu_onset_fkey.restype = ctypes.c_uint
        _lib.emu_onset_strength_f32.argtypes = [_p, _i64, _i64, _i64, _i64, _p, _i64, _int, _int, _int, _int, _f, _f, _f, _f,
                                                _p, _p, _i64, _int]
        _lib.emu_onset_db_values.argtypes = [_p, _i64, _f, _f, _f, _f, _p, _p]
        _lib.emu_peak_pick_f32.argtypes = [_p, _i64, _i64, _i64, _int, _int, _int, _int, _f, _int, _int, _int, _int, _p,
                                           _i64, _p, _p, _int]
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_onset_last_error().decode())


def last_error():
    return lib().emu_onset_last_error().decode()


def geometry():
    g = lib().emu_onset_geometry()
    return dict(staged=g[0], n_tt=g[1], lds_bytes=g[2])


def lds_overruns():
    return int(lib().emu_onset_lds_overruns())


def max_frames():
    return int(lib().emu_peak_pick_max_frames())


class _Guarded:
    """A (..., rs) float32 buffer between two NaN bands, its pad columns T .. rs - 1 NaN as well."""

    def __init__(self, lead, T, rs, data=None):
        self.shape, self.T = tuple(lead) + (rs,), T
        n = int(np.prod(self.shape))
        self.raw = np.full(n + 2 * BAND, np.nan, np.float32)
        self.body = self.raw[BAND:BAND + n].reshape(self.shape)
        if data is not None:
            self.body[..., :T] = data
        self.ptr = self.raw.ctypes.data + 4 * BAND

    def intact(self, written):
        """The bands and the pad columns are still NaN; `written`: the payload holds no NaN any more."""
        ok = np.isnan(self.raw[:BAND]).all() and np.isnan(self.raw[-BAND:]).all() and np.isnan(self.body[..., self.T:]).all()
        return bool(ok and (not written or not np.isnan(self.body[..., :self.T]).any()))


def _db_args(db):
    """(mode, coef, amin, ref, top_db, key array or None) of db = None | dict(smax=..., top_db=80.0, ...)."""
    if db is None:
        return 0, 10.0, 1e-10, 1.0, -1.0, None
    top_db = db.get("top_db", 80.0)
    key = np.array([lib().emu_onset_fkey(float(np.float32(db["smax"])))], np.uint32)
    return 1, db.get("coef", 10.0), db.get("amin", 1e-10), db.get("ref", 1.0), -1.0 if top_db is None else top_db, key


def db_values(S, db):
    """The float32 dB values the kernel computes on load, through the same ap_db_* helpers."""
    S = np.ascontiguousarray(S, np.float32)
    out = np.empty_like(S)
    _, coef, amin, ref, top_db, key = _db_args(db)
    _check(lib().emu_onset_db_values(S.ctypes.data, S.size, coef, amin, ref, top_db, key.ctypes.data, out.ctypes.data))
    return out


def onset_strength(S, *, lag=1, max_size=1, shift=None, ref=None, db=None, pad_in=0, pad_ref=0, pad_out=0, grid=0):
    """out (B, T) of a (B, M, T) float32 array through the emulated C entry.  pad_*: extra (NaN) columns per row of the
    input / the reference / the output.  Asserts that no band or pad column was written and that no NaN came out:
    a read of a band or a pad column would put one there, because the kernel's window maximum and its rectification
    keep a NaN (test_emu_onset_strength_nan_guard_is_live).  Not in dB mode: max(s, amin) of the conversion drops a NaN
    by definition, so there the guard covers writes, and the reads are the same index arithmetic as without dB."""
    S = np.asarray(S, np.float32)
    B, M, T = S.shape
    src = _Guarded((B, M), T, T + pad_in, S)
    rsrc = None if ref is None else _Guarded((B, M), T, T + pad_ref, np.asarray(ref, np.float32))
    out = _Guarded((B,), T, T + pad_out)
    mode, coef, amin, dref, top_db, key = _db_args(db)
    _check(lib().emu_onset_strength_f32(src.ptr, B, M, T, T + pad_in, None if rsrc is None else rsrc.ptr, T + pad_ref,
                                        lag, max_size, lag if shift is None else shift, mode, coef, amin, dref, top_db,
                                        None if key is None else key.ctypes.data, out.ptr, T + pad_out, grid))
    assert out.intact(written=True), "a band or a pad column was written, or a value is NaN"
    assert src.intact(written=False) and (rsrc is None or rsrc.intact(written=False))
    return out.body[:, :T].copy()


def strength_raw(S_ptr, B, M, T, rs, ref_ptr, rs_ref, lag, max_size, shift, db_mode, top_db, key_ptr, out_ptr, rs_out):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_onset_strength_f32(S_ptr, B, M, T, rs, ref_ptr, rs_ref, lag, max_size, shift, db_mode, 10.0, 1e-10, 1.0,
                                        top_db, key_ptr, out_ptr, rs_out, 0)


def peak_pick(x, *, pre_max, post_max, pre_avg, post_avg, delta, wait, normalize=False, guard=False, backtrack=False,
              energy=None, pad_in=0, grid=0):
    """(mask (B, T) bool, count (B,)) of a (B, T) float32 array through the emulated C entry; x may hold NaN."""
    x = np.asarray(x, np.float32)
    B, T = x.shape
    src = _Guarded((B,), T, T + pad_in, x)
    esrc = None if energy is None else _Guarded((B,), T, T + pad_in, np.asarray(energy, np.float32))
    raw = np.full(B * T + 2 * BAND, 0xFF, np.uint8)
    cnt = np.full(B + 2, -7, np.int32)
    _check(lib().emu_peak_pick_f32(src.ptr, B, T, T + pad_in, pre_max, post_max, pre_avg, post_avg, float(delta), wait,
                                   int(normalize), int(guard), int(backtrack), None if esrc is None else esrc.ptr, T + pad_in,
                                   raw.ctypes.data + BAND, cnt.ctypes.data + 4, grid))
    assert (raw[:BAND] == 0xFF).all() and (raw[-BAND:] == 0xFF).all() and cnt[0] == -7 and cnt[-1] == -7, "a band was written"
    assert np.isnan(src.raw[:BAND]).all() and np.isnan(src.raw[-BAND:]).all() and np.isnan(src.body[:, T:]).all()
    mask = raw[BAND:BAND + B * T].reshape(B, T)
    assert set(np.unique(mask)) <= {0, 1}
    assert np.array_equal(mask.sum(axis=1), cnt[1:-1])
    return mask.astype(bool), cnt[1:-1].copy()


def peak_pick_raw(x_ptr, B, T, rs, pre_max, post_max, pre_avg, post_avg, wait, mask_ptr):
    return lib().emu_peak_pick_f32(x_ptr, B, T, rs, pre_max, post_max, pre_avg, post_avg, 0.0, wait, 0, 0, 0, None, 0, mask_ptr,
                                   None, 0)
