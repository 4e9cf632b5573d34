"""ctypes bindings for tests/emu/libapemu_istft_stream.so (TEST INFRASTRUCTURE ONLY).

Runs the streaming ISTFT kernel source (kernels_istft_stream.h) on the CPU through the SIMT emulator of
emu_shim.h.  Built on demand with g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_istft_stream.so")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int


def build(force=False):
    srcs = [os.path.join(HERE, "emu_istft_stream.cpp"), os.path.join(CSRC, "host_builders.cpp")]
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
        _lib.emu_istft_stream_last_error.restype = ctypes.c_char_p
        _lib.ap_twiddle_table_host.argtypes = [_int, _p]
        _lib.emu_istft_stream_f32.argtypes = [_p, _i64, _i64, _i64, _int, _int, _p, _p, _i64, _p, _p, _int,
                                              _i64, _i64, _p, _p, _int]
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _check(rc):
    if rc != 0:
        raise ValueError(lib().emu_istft_stream_last_error().decode())


def twiddles(n_fft):
    tw = np.empty(2 * n_fft, np.float32)
    _check(lib().ap_twiddle_table_host(n_fft, tw.ctypes.data))
    return tw


class Stream:
    """StreamingISTFT's call sequence over the emulated C entry: host buffers, G frames per workgroup."""

    def __init__(self, n_fft, hop, window, center=False, G=2):
        self.n, self.hop, self.center, self.G = n_fft, hop, center, G
        self.window = np.ascontiguousarray(window, np.float32)
        self.tw = twiddles(n_fft)
        self.K = 0
        self.B = 1
        self.carry = None

    def _call(self, S, T, final):
        n, hop = self.n, self.hop
        off = n // 2 if self.center else 0
        B = self.B
        lo = max(self.K * hop, off)
        hi = max((self.K + T - 1) * hop + n - off if final else (self.K + T) * hop, lo)
        out = np.empty((B, hi - lo), np.float32)
        carry_out = np.empty((B, max(n - hop, 1)), np.float32)
        ws = np.empty(B * T * n, np.float32) if (T and n not in (2048, 1024, 512, 400, 256)) else None
        Sr, rs = (None, 0) if S is None else S
        _check(lib().emu_istft_stream_f32(_ptr(Sr), B, T, rs, n, hop, _ptr(self.window), _ptr(self.tw), self.K,
                                          _ptr(self.carry), _ptr(carry_out), int(final), lo, hi, _ptr(ws),
                                          _ptr(out), self.G))
        self.carry = carry_out
        self.K += T
        return out

    def process(self, S, row_stride=None):
        """S: complex (B, F, T); row_stride > T lays the rows out that far apart (line-padded views)."""
        B, F, T = S.shape
        self.B = B
        rs = T if row_stride is None else row_stride
        buf = np.zeros((B, F, max(rs, 1), 2), np.float32)
        buf[:, :, :T, 0] = S.real
        buf[:, :, :T, 1] = S.imag
        return self._call((buf, rs), T, False)

    def flush(self):
        return self._call(None, 0, True)
