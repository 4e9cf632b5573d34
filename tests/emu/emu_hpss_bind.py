"""ctypes bindings for tests/emu/libapemu_hpss.so (TEST INFRASTRUCTURE ONLY).

Runs the HPSS kernel source (kernels_hpss.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_hpss.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float

BAND = 64          # NaN floats before and after every buffer


def build(force=False):
    srcs = [os.path.join(HERE, "emu_hpss.cpp")]
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
        _lib.emu_hpss_last_error.restype = ctypes.c_char_p
        _lib.emu_hpss_geometry.restype = ctypes.POINTER(ctypes.c_int)
        _lib.emu_hpss_fused.argtypes = [_int, _int]
        _lib.emu_hpss_f32.argtypes = [_p, _int, _i64, _i64, _i64, _i64, _int, _int, _f, _f, _f, _int, _int, _p, _p,
                                      _i64, _int, _int]
    return _lib


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_hpss_last_error().decode())


def last_error():
    return lib().emu_hpss_last_error().decode()


def geometry():
    g = lib().emu_hpss_geometry()
    return dict(fused=g[0], f_tile=g[1], n_ft=g[2], n_tt=g[3], lds_bytes=g[4])


def lds_overruns():
    return int(lib().emu_hpss_lds_overruns())


def network():
    return int(lib().emu_hpss_net_comparators()), int(lib().emu_hpss_net_ops())


def default_tile():
    return int(lib().emu_hpss_default_tile())


class _Guarded:
    """A (B, F, rs[, 2]) float32 buffer between two NaN bands, its pad columns T .. rs - 1 NaN as well."""

    def __init__(self, B, F, T, rs, width, data=None):
        self.shape, self.T = (B, F, rs) + ((2,) if width == 2 else ()), T
        n = int(np.prod(self.shape))
        self.raw = np.full(n + 2 * BAND, np.nan, np.float32)
        self.body = self.raw[BAND:BAND + n].reshape(self.shape)
        if data is not None:
            self.body[:, :, :T] = data
        self.ptr = self.raw.ctypes.data + 4 * BAND

    def intact(self, written):
        """The bands and the pad columns are still NaN; `written`: the payload holds no NaN any more / only NaN."""
        ok = np.isnan(self.raw[:BAND]).all() and np.isnan(self.raw[-BAND:]).all() and np.isnan(self.body[:, :, self.T:]).all()
        pay = np.isnan(self.body[:, :, :self.T])
        return bool(ok and (not pay.any() if written else pay.all()))


def hpss(S, *, kernel_size=(31, 31), margin=(1.0, 1.0), power=2.0, mode=0, general=False, f_tile=0, grid=0,
         pad_in=0, pad_out=0, want=(True, True)):
    """(out_h, out_p) of a (B, F, T) float32 / complex64 array through the emulated C entry; None for an output not
    asked for.  pad_in / pad_out: extra (NaN) columns per row of the input / the outputs.  Asserts that no band, pad
    column or unwanted output was written; a read of one would put NaN into the results."""
    S = np.asarray(S)
    cplx = np.iscomplexobj(S)
    S = S.astype(np.complex64 if cplx else np.float32)
    B, F, T = S.shape
    win = 2 if cplx else 1
    wout = 2 if (cplx and mode == 0) else 1
    src = _Guarded(B, F, T, T + pad_in, win, np.stack([S.real, S.imag], -1) if cplx else S)
    outs = [_Guarded(B, F, T, T + pad_out, wout) for _ in range(2)]
    kh, kp = kernel_size
    _check(lib().emu_hpss_f32(src.ptr, int(cplx), B, F, T, T + pad_in, kh, kp, float(margin[0]), float(margin[1]),
                              float(power), mode, int(general), outs[0].ptr if want[0] else None,
                              outs[1].ptr if want[1] else None, T + pad_out, f_tile, grid))
    res = []
    for o, w in zip(outs, want):
        assert o.intact(written=w), "a band, a pad column or an output that was not asked for was written (or a value is NaN)"
        if not w:
            res.append(None)
        else:
            v = o.body[:, :, :T].copy()
            res.append(v[..., 0] + 1j * v[..., 1] if wout == 2 else v)
    if wout == 2:
        res = [None if r is None else r.astype(np.complex64) for r in res]
    return res[0], res[1]


def raw_call(S_ptr, is_complex, B, F, T, rs_in, kh, kp, mh, mp, power, mode, general, out_h, out_p, rs_out, f_tile=0):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_hpss_f32(S_ptr, is_complex, B, F, T, rs_in, kh, kp, mh, mp, power, mode, general, out_h, out_p,
                              rs_out, f_tile, 0)
