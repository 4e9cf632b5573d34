"""ctypes bindings for tests/emu/libapemu_chroma.so (TEST INFRASTRUCTURE ONLY).

Runs the chroma kernel source (kernels_chroma.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_chroma.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float

BAND = 64          # NaN floats before and after every float buffer
NORMS = {None: 0, 1: 1, 2: 2, np.inf: 3}


def build(force=False):
    srcs = [os.path.join(HERE, "emu_chroma.cpp")]
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
        _lib.emu_chroma_last_error.restype = ctypes.c_char_p
        _lib.emu_chroma_geometry.restype = ctypes.POINTER(ctypes.c_int)
        _lib.emu_chroma_fold_f32.argtypes = [_p, _int, _i64, _int, _i64, _i64, _p, _int, _int, _int, _f, _int, _p, _i64, _int]
        _lib.emu_chroma_cens_f32.argtypes = [_p, _i64, _int, _i64, _i64, _p, _int, _int, _p, _i64, _int]
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_chroma_last_error().decode())


def last_error():
    return lib().emu_chroma_last_error().decode()


def constants():
    """The tile constants of kernels_chroma.h."""
    g = lib().emu_chroma_geometry()
    return dict(fold_tile=g[0], fold_waves=g[1], fold_run=g[2], max_out=g[3], cens_tile=g[4], max_smooth=g[5], cens_threads=g[6])


def geometry():
    """What the prepare step chose for the last call."""
    g = lib().emu_chroma_geometry()
    return dict(accumulators=g[7], grid=g[8], lds_bytes=g[9])


def _guarded(a):
    """(raw array with NaN bands, pointer to the payload) of a float32 array."""
    a = np.ascontiguousarray(a, np.float32).ravel()
    raw = np.full(a.size + 2 * BAND, np.nan, np.float32)
    raw[BAND:BAND + a.size] = a
    return raw, raw.ctypes.data + 4 * BAND


def _rows_in(x, pad, complex_in):
    """x (B, K, T) laid out with `pad` NaN columns behind every row: (raw, pointer, row stride in elements)."""
    B, K, T = x.shape
    rs = T + pad
    if complex_in:
        body = np.full((B, K, rs), complex(np.nan, np.nan), np.complex64)
        body[:, :, :T] = x
        raw, ptr = _guarded(body.view(np.float32))
    else:
        body = np.full((B, K, rs), np.nan, np.float32)
        body[:, :, :T] = x
        raw, ptr = _guarded(body)
    return raw, ptr, rs


def _collect(oraw, B, n, T, rs, allow_nan):
    body = oraw[BAND:-BAND].reshape(B, n, rs)
    assert lib().emu_chroma_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"
    assert np.isnan(oraw[:BAND]).all() and np.isnan(oraw[-BAND:]).all() and np.isnan(body[:, :, T:]).all(), \
        "a band or a pad column was written"
    got = body[:, :, :T].copy()
    if not allow_nan:
        assert not np.isnan(got).any(), "a value is NaN or was not written"
    return got


def fold(x, w, *, in_kind=None, pre_l1=False, threshold=None, norm=None, pad_in=0, pad_out=0, grid=0, allow_nan=False):
    """out (B, n_out, T) float32 of x (B, K, T) float32 / complex64 through the emulated C entry.  w: (n_out, K) or None
    (the identity).  in_kind: 0 for real x; 1 or 2 for complex x (default 1).  pad_in / pad_out: NaN columns behind
    every input / output row.  Asserts that no band and no pad column was written and (unless allow_nan) that every
    payload value was written and none is NaN: x and w lie between NaN bands and NaN pad columns, so a read outside
    either would put a NaN into a sum."""
    x = np.asarray(x)
    cplx = np.iscomplexobj(x)
    kind = (1 if in_kind is None else in_kind) if cplx else 0
    x = x.astype(np.complex64 if cplx else np.float32)
    B, K, T = x.shape
    xraw, xptr, in_rs = _rows_in(x, pad_in, cplx)
    if w is None:
        n_out, wraw, wptr = K, None, None
    else:
        w = np.ascontiguousarray(w, np.float32)
        n_out = w.shape[0]
        assert w.shape == (n_out, K)
        wraw, wptr = _guarded(w)
    rs = T + pad_out
    oraw = np.full(B * n_out * rs + 2 * BAND, np.nan, np.float32)
    _check(lib().emu_chroma_fold_f32(xptr, kind, B, K, T, in_rs, wptr, n_out, int(bool(pre_l1)), int(threshold is not None),
                                     float(threshold or 0.0), NORMS[norm], oraw.ctypes.data + 4 * BAND, rs, int(grid)))
    return _collect(oraw, B, n_out, T, rs, allow_nan)


def cens(x, taps, *, norm=2, pad_in=0, pad_out=0, grid=0, allow_nan=False):
    """out (B, n, T) float32 of chroma x (B, n, T) through the emulated C entry; taps: 1-D float32 or None."""
    x = np.asarray(x, np.float32)
    B, n, T = x.shape
    xraw, xptr, in_rs = _rows_in(x, pad_in, False)
    n_taps = 0 if taps is None else len(taps)
    traw, tptr = (None, None) if n_taps == 0 else _guarded(taps)
    rs = T + pad_out
    oraw = np.full(B * n * rs + 2 * BAND, np.nan, np.float32)
    _check(lib().emu_chroma_cens_f32(xptr, B, n, T, in_rs, tptr, n_taps, NORMS[norm], oraw.ctypes.data + 4 * BAND, rs, int(grid)))
    return _collect(oraw, B, n, T, rs, allow_nan)


def fold_raw(x_ptr, in_kind, B, K, T, in_rs, w_ptr, n_out, norm, out_ptr, out_rs):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_chroma_fold_f32(x_ptr, in_kind, B, K, T, in_rs, w_ptr, n_out, 0, 0, 0.0, norm, out_ptr, out_rs, 0)


def cens_raw(x_ptr, B, n, T, in_rs, taps_ptr, n_taps, norm, out_ptr, out_rs):
    return lib().emu_chroma_cens_f32(x_ptr, B, n, T, in_rs, taps_ptr, n_taps, norm, out_ptr, out_rs, 0)
