"""ctypes bindings for tests/emu/libapemu_nmf.so (TEST INFRASTRUCTURE ONLY).

Runs the NMF kernel source (kernels_nmf.h) on the CPU through the SIMT emulator of emu_shim.h and the MFMA model of
emu_mfma.h.  Built on demand with g++; never imported by the product package.  Every buffer lies between poisoned
bands, the rows of V have NaN pad columns behind them, and LDS beyond the bytes the host asked for is watched."""

from __future__ import annotations

import ctypes
import os

import numpy as np

from emu_viterbi_bind import BAND, CSRC, HERE, ROOT, compile_lib

LIB = os.path.join(HERE, "libapemu_nmf.so")
SRC = os.path.join(HERE, "emu_nmf.cpp")
LOSS = {"frobenius": 0, "kullback-leibler": 1}

_p, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(HERE, "emu_shim.h"), os.path.join(HERE, "emu_mfma.h"), os.path.join(ROOT, "include", "audioprims.h"),
                os.path.join(CSRC, "kernels_nmf.h"), os.path.join(CSRC, "ap_launch.h")]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            compile_lib(LIB, SRC)
        L = ctypes.CDLL(LIB)
        L.emu_nmf_last_error.restype = ctypes.c_char_p
        L.emu_nmf_workspace_bytes.restype = _i64
        L.emu_nmf_workspace_bytes.argtypes = [_i64, _i64, _int]
        L.emu_nmf_mu_f32.argtypes = [_p, _i64, _i64, _i64, _i64, _int, _p, _p, _int, _int, _int, ctypes.c_float, _p, _int]
        L.emu_nmf_objective_f32.argtypes = [_p, _i64, _i64, _i64, _i64, _int, _p, _p, _int, ctypes.c_float, _p, _p, _int]
        _lib = L
    return _lib


def _guarded(a, dtype=np.float32):
    """(raw array with NaN bands, pointer to the payload) holding a copy of `a`."""
    a = np.ascontiguousarray(a, dtype).ravel()
    raw = np.full(a.size + 2 * BAND, np.nan, dtype)
    raw[BAND:BAND + a.size] = a
    return raw, raw.ctypes.data + raw.itemsize * BAND


def _payload(raw, shape, what):
    assert np.isnan(raw[:BAND]).all() and np.isnan(raw[-BAND:]).all(), f"{what}: a band was written"
    assert lib().emu_nmf_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"
    return raw[BAND:-BAND].reshape(shape).copy()


def _call(V, W, H, loss, pad, fn):
    B, F, T = V.shape
    K = W.shape[-1]
    body = np.full((B, F, T + pad), np.nan, np.float32)
    body[:, :, :T] = V
    vraw, vptr = _guarded(body)
    wraw, wptr = _guarded(W)
    hraw, hptr = _guarded(H)
    sraw, sptr = _guarded(np.zeros(int(lib().emu_nmf_workspace_bytes(B, T, K)) // 8), np.float64)
    rc = fn(vptr, B, F, T, T + pad, K, wptr, hptr, LOSS[loss], sptr)
    if rc != 0:
        raise ValueError(lib().emu_nmf_last_error().decode())
    _payload(sraw, (-1,), "workspace")
    assert np.array_equal(_payload(vraw, body.shape, "V"), body, equal_nan=True)
    return _payload(wraw, W.shape, "W"), _payload(hraw, H.shape, "H")


def mu(V, W, H, loss, *, n_iter=1, update_w=True, eps=1e-10, pad=3, grid=0):
    """(W, H) after n_iter multiplicative updates through the emulated C entry; `pad` NaN columns behind every row of V."""
    return _call(V, W, H, loss, pad, lambda v, B, F, T, rs, K, w, h, l, s: lib().emu_nmf_mu_f32(
        v, B, F, T, rs, K, w, h, int(n_iter), l, int(update_w), eps, s, int(grid)))


def objective(V, W, H, loss, *, eps=1e-10, pad=3, grid=0):
    """The objective per item, float64 (B)."""
    oraw, optr = _guarded(np.zeros(V.shape[0]), np.float64)
    _call(V, W, H, loss, pad, lambda v, B, F, T, rs, K, w, h, l, s: lib().emu_nmf_objective_f32(
        v, B, F, T, rs, K, w, h, l, eps, optr, s, int(grid)))
    return _payload(oraw, (V.shape[0],), "objective")
