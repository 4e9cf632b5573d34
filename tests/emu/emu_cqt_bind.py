"""ctypes bindings for tests/emu/libapemu_cqt.so (TEST INFRASTRUCTURE ONLY).

Runs the constant-Q kernel source (kernels_cqt.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_cqt.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int

BAND = 64          # NaN floats before and after every float buffer
PAD_MODES = {"constant": 0, "edge": 1, "reflect": 2}


def build(force=False):
    srcs = [os.path.join(HERE, "emu_cqt.cpp")]
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
        _lib.emu_cqt_last_error.restype = ctypes.c_char_p
        _lib.emu_cqt_geometry.restype = ctypes.POINTER(ctypes.c_int)
        _lib.emu_cqt_f32.argtypes = [_p, _i64, _i64, _int, _int, _p, _p, _p, _p, _int, _i64, _p, _i64, _int]
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_cqt_last_error().decode())


def last_error():
    return lib().emu_cqt_last_error().decode()


def geometry():
    """The tile constants of kernels_cqt.h and what ap_prepare_cqt chose for the last call."""
    g = lib().emu_cqt_geometry()
    return dict(frames_per_tile=g[0], bins_per_group=g[1], chunk=g[2], lanes=g[3], reduction_chain=g[4], n_groups=g[5],
                n_tt=g[6], grid=g[7], lds_bytes=g[8], max_taps=g[9])


def constants():
    """The tile constants alone (a call that validates and launches nothing sets them too late: one tiny launch)."""
    if lib().emu_cqt_geometry()[0] == 0:
        one = np.ones(1, np.complex64)
        cqt(np.zeros((1, 1), np.float32), 1, "constant", one, np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.float32))
    g = geometry()
    return {k: g[k] for k in ("frames_per_tile", "bins_per_group", "chunk", "lanes", "reduction_chain", "max_taps")}


def _guarded(a):
    """(raw array with NaN bands, pointer to the payload) of a float32 array."""
    a = np.ascontiguousarray(a, np.float32).ravel()
    raw = np.full(a.size + 2 * BAND, np.nan, np.float32)
    raw[BAND:BAND + a.size] = a
    return raw, raw.ctypes.data + 4 * BAND


def cqt(y, hop, pad_mode, taps, tap_offset, m0, scale, *, pad_out=0, grid=0):
    """C (B, n_bins, T) complex64 of y (B, L) float32 through the emulated C entry.  taps: complex64, back to back;
    pad_out: extra (NaN) complex columns per output row.  Asserts that no band and no pad column was written, that
    every payload value was, and that none is NaN: the signal and the taps lie between NaN bands, so a read outside
    either would put a NaN into a sum."""
    y = np.asarray(y, np.float32)
    B, L = y.shape
    n_bins = len(m0)
    T = 1 + L // int(hop)
    rs = T + pad_out
    taps = np.ascontiguousarray(taps, np.complex64)
    yraw, yptr = _guarded(y)
    traw, tptr = _guarded(taps.view(np.float32))
    sraw, sptr = _guarded(scale)
    off = np.ascontiguousarray(tap_offset, np.int64)
    m0 = np.ascontiguousarray(m0, np.int32)
    assert off.shape == (n_bins + 1,) and off[-1] == taps.size
    oraw = np.full(2 * B * n_bins * rs + 2 * BAND, np.nan, np.float32)
    body = oraw[BAND:-BAND].reshape(B, n_bins, rs, 2)
    _check(lib().emu_cqt_f32(yptr, B, L, int(hop), PAD_MODES[pad_mode], tptr, off.ctypes.data, m0.ctypes.data, sptr, n_bins,
                             T, oraw.ctypes.data + 4 * BAND, rs, int(grid)))
    assert lib().emu_cqt_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"
    assert np.isnan(oraw[:BAND]).all() and np.isnan(oraw[-BAND:]).all() and np.isnan(body[:, :, T:]).all(), \
        "a band or a pad column was written"
    got = body[:, :, :T].copy()
    assert not np.isnan(got).any(), "a value is NaN or was not written"
    return np.ascontiguousarray(got).view(np.complex64)[..., 0]


def cqt_raw(y_ptr, B, L, hop, pad_mode, taps_ptr, off_ptr, m0_ptr, scale_ptr, n_bins, T, out_ptr, rs):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_cqt_f32(y_ptr, B, L, hop, pad_mode, taps_ptr, off_ptr, m0_ptr, scale_ptr, n_bins, T, out_ptr, rs, 0)
