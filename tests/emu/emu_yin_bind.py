"""ctypes bindings for tests/emu/libapemu_yin.so (TEST INFRASTRUCTURE ONLY).

Runs the YIN kernel source (kernels_yin.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand
with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_yin.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float


def build(force=False):
    srcs = [os.path.join(HERE, "emu_yin.cpp"), os.path.join(CSRC, "host_builders.cpp")]
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
        _lib.emu_yin_last_error.restype = ctypes.c_char_p
        _lib.ap_twiddle_table_host.argtypes = [_int, _p]
        _lib.emu_yin_fused.argtypes = [_int, _int, _i64]
        _lib.emu_yin_f32.argtypes = [_p, _i64, _i64, _int, _int, _int, _int, _int, _f, _f, _p, _p, _p, _int]
        _lib.emu_yin_cmnd_f32.argtypes = [_p, _i64, _i64, _int, _int, _int, _int, _int, _p, _p, _int]
    return _lib


def _check(rc):
    if rc != 0:
        raise ValueError(lib().emu_yin_last_error().decode())


def twiddles(n):
    tw = np.empty(2 * n, np.float32)
    _check(lib().ap_twiddle_table_host(n, tw.ctypes.data))
    return tw


def lag_range(sr, fmin, fmax, frame_length):
    lo = max(int(math.floor(sr / fmax)), 1)
    hi = min(int(math.ceil(sr / fmin)), frame_length - frame_length // 2 - 1)
    return lo, hi


def _prep(y, frame_length, hop, general):
    y = np.ascontiguousarray(np.atleast_2d(y), np.float32)
    B, L = y.shape
    fused = (not general) and bool(lib().emu_yin_fused(frame_length, hop, L))
    tw = twiddles(frame_length) if fused else None
    return y, B, L, tw


def yin(y, *, fmin, fmax, sr=22050, frame_length=2048, hop_length=None, trough_threshold=0.1, center=True,
        general=False, grid=0):
    """(f0, aperiodicity, served by the wave kernel?) of a (B, L) batch through the emulated C entry."""
    hop = frame_length // 4 if hop_length is None else hop_length
    y, B, L, tw = _prep(y, frame_length, hop, general)
    lo, hi = lag_range(sr, fmin, fmax, frame_length)
    T = 1 + (L + (2 * (frame_length // 2) if center else 0) - frame_length) // hop
    f0 = np.full((B, max(T, 0)), np.nan, np.float32)
    ap = np.full((B, max(T, 0)), np.nan, np.float32)
    _check(lib().emu_yin_f32(y.ctypes.data, B, L, frame_length, hop, int(center), lo, hi, float(sr),
                             float(trough_threshold), None if tw is None else tw.ctypes.data, f0.ctypes.data,
                             ap.ctypes.data, grid))
    return f0, ap, tw is not None


def yin_cmnd(y, *, fmin, fmax, sr=22050, frame_length=2048, hop_length=None, center=True, general=False, grid=0):
    hop = frame_length // 4 if hop_length is None else hop_length
    y, B, L, tw = _prep(y, frame_length, hop, general)
    lo, hi = lag_range(sr, fmin, fmax, frame_length)
    T = 1 + (L + (2 * (frame_length // 2) if center else 0) - frame_length) // hop
    out = np.full((B, hi - lo + 1, max(T, 0)), np.nan, np.float32)
    _check(lib().emu_yin_cmnd_f32(y.ctypes.data, B, L, frame_length, hop, int(center), lo, hi,
                                  None if tw is None else tw.ctypes.data, out.ctypes.data, grid))
    return out, tw is not None


def lds_overruns():
    return int(lib().emu_yin_lds_overruns())
