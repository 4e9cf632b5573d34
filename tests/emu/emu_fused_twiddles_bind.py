"""ctypes bindings for tests/emu/libapemu_fused_twiddles.so (TEST INFRASTRUCTURE ONLY).

The scalar twins of the fused twiddle primitives of csrc/fft_lds.h on host values.  Built on demand with g++; never
imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_fused_twiddles.so")

_f32p = ctypes.POINTER(ctypes.c_float)


def build(force=False):
    srcs = [os.path.join(HERE, "emu_fused_twiddles.cpp")]
    deps = srcs + [os.path.join(HERE, "emu_shim.h")] + [os.path.join(CSRC, f) for f in ("fft_lds.h", "ap_common.h")]
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
        _lib.emu_fused_twiddle_prims.argtypes = [_f32p, ctypes.c_int64] + [ctypes.c_float] * 4 + [_f32p]
    return _lib


def prims(rec, ca, ta, cb, tb):
    """(n, 6, 2) float32 records (a, b, x2, x3, wa, wb) -> (n, 24, 2): see emu_fused_twiddles.cpp."""
    rec = np.ascontiguousarray(rec, np.float32)
    n = rec.shape[0]
    out = np.zeros((n, 24, 2), np.float32)
    rc = lib().emu_fused_twiddle_prims(rec.ctypes.data_as(_f32p), n, ca, ta, cb, tb, out.ctypes.data_as(_f32p))
    assert rc == 0
    return out
