"""ctypes bindings for tests/emu/libapemu_pcen.so (TEST INFRASTRUCTURE ONLY).

Runs the PCEN kernel source (kernels_pcen.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_pcen.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float

BAND = 64          # NaN floats before and after every buffer


def build(force=False):
    srcs = [os.path.join(HERE, "emu_pcen.cpp")]
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
        _lib.emu_pcen_last_error.restype = ctypes.c_char_p
        _lib.emu_pcen_geometry.restype = ctypes.POINTER(ctypes.c_int)
        _lib.emu_pcen_f32.argtypes = [_p, _i64, _i64, _i64, _i64, _p, _i64, _int, ctypes.c_double, _f, _f, _f, _f, _p, _p,
                                      _i64, _p, _int]
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_pcen_last_error().decode())


def last_error():
    return lib().emu_pcen_last_error().decode()


def geometry():
    g = lib().emu_pcen_geometry()
    return dict(chain=g[0], n_tt=g[1], grid=g[2])


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

    def intact(self):
        """The bands and the pad columns are still NaN."""
        return bool(np.isnan(self.raw[:BAND]).all() and np.isnan(self.raw[-BAND:]).all() and np.isnan(self.body[..., self.T:]).all())


def pcen(S, *, b, gain=0.98, bias=2.0, power=0.5, eps=1e-6, max_size=1, ref=None, zi=None, want_zf=True, pad_in=0,
         pad_ref=0, pad_out=0, grid=0, allow_nan=False):
    """(out (B, M, T), zf (B, M) or None) of a (B, M, T) float32 array through the emulated C entry.  pad_*: extra (NaN)
    columns per row of the input / the reference / the output; zi: None or (B, M).  Asserts that no band or pad column
    was written and, unless allow_nan, that every value was written and none is NaN: a read of a band or a pad column
    would put one there, because the window maximum, the scan and the chain keep a NaN
    (test_emu_pcen_nan_reaches_later_frames_of_the_window_only)."""
    S = np.asarray(S, np.float32)
    B, M, T = S.shape
    src = _Guarded((B, M), T, T + pad_in, S)
    rsrc = None if ref is None else _Guarded((B, M), T, T + pad_ref, np.asarray(ref, np.float32))
    out = _Guarded((B, M), T, T + pad_out)
    zin = None if zi is None else _Guarded((B,), M, M, np.broadcast_to(np.asarray(zi, np.float32), (B, M)))
    zout = _Guarded((B,), M, M) if want_zf else None
    _check(lib().emu_pcen_f32(src.ptr, B, M, T, T + pad_in, None if rsrc is None else rsrc.ptr, T + pad_ref, int(max_size),
                              float(b), gain, bias, power, eps, None if zin is None else zin.ptr, out.ptr, T + pad_out,
                              None if zout is None else zout.ptr, grid))
    assert out.intact() and (zout is None or zout.intact()), "a band or a pad column was written"
    assert src.intact() and (rsrc is None or rsrc.intact()) and (zin is None or zin.intact())
    got = out.body[..., :T].copy()
    zf = None if zout is None else zout.body.copy()
    if not allow_nan:
        assert not np.isnan(got).any() and (zf is None or not np.isnan(zf).any()), "a value is NaN or was not written"
    return got, zf


def pcen_raw(S_ptr, B, M, T, rs, ref_ptr, rs_ref, max_size, b, gain, bias, power, eps, zi_ptr, out_ptr, rs_out, zf_ptr):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_pcen_f32(S_ptr, B, M, T, rs, ref_ptr, rs_ref, max_size, b, gain, bias, power, eps, zi_ptr, out_ptr,
                              rs_out, zf_ptr, 0)
