"""ctypes bindings for tests/emu/libapemu_dtw.so (TEST INFRASTRUCTURE ONLY).

Runs the DTW kernel source (kernels_dtw.h) on the CPU through the SIMT emulator of emu_shim.h.  Built on demand with
g++; never imported by the product package."""

from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "mlx-audio-primitives_amd", "csrc")
LIB = os.path.join(HERE, "libapemu_dtw.so")
SRC = os.path.join(HERE, "emu_dtw.cpp")

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int

BAND = 64           # poisoned elements before and after every buffer
BYTE_POISON = 0xEE  # of uint8 buffers: no step code
METRICS = {"euclidean": 0, "sqeuclidean": 1, "cityblock": 2, "cosine": 3}


def compile_lib(out, src=SRC, include_dirs=()):
    tmp = f"{out}.{os.getpid()}.tmp"
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-pthread", "-I", HERE] + [f"-I{d}" for d in include_dirs]
                          + ["-o", tmp, src])
    os.replace(tmp, out)
    return out


def build(force=False):
    deps = [SRC, os.path.join(HERE, "emu_shim.h"), os.path.join(ROOT, "include", "audioprims.h")] + [
        os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")
    ]
    if not force and os.path.exists(LIB):
        if os.path.getmtime(LIB) >= max(os.path.getmtime(d) for d in deps):
            return LIB
    return compile_lib(LIB)


def declare(L):
    L.emu_dtw_last_error.restype = ctypes.c_char_p
    L.emu_dtw_geometry.restype = ctypes.POINTER(ctypes.c_int)
    L.emu_dtw_cost_f32.argtypes = [_p, _p, _i64, _int, _i64, _i64, _i64, _i64, _int, _p, _i64, _int]
    L.emu_dtw_accumulate_f32.argtypes = [_p, _i64, _i64, _i64, _i64, _int, _p, _p, _p, _int, _int, _i64, _p, _i64, _p, _i64, _int]
    L.emu_dtw_backtrack_i32.argtypes = [_p, _p, _p, _i64, _i64, _i64, _i64, _i64, _int, _p, _int, _p, _p, _int]
    return L


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = declare(ctypes.CDLL(build()))
    return _lib


def use(handle):
    """Route every call through another build of the twin (the mutation tests); None: the regular one."""
    global _lib
    _lib = handle


class Status(ValueError):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _check(rc):
    if rc != 0:
        raise Status(rc, lib().emu_dtw_last_error().decode())


def last_error():
    return lib().emu_dtw_last_error().decode()


def constants():
    """The constants of kernels_dtw.h."""
    g = lib().emu_dtw_geometry()
    names = ("tile_w", "tile_h", "waves", "halo_rows", "halo_cols", "max_steps", "max_step", "max_len", "cost_tile_rows",
             "cost_tile_cols", "cost_chunk", "max_features", "window")
    return {n: g[i] for i, n in enumerate(names)}


def geometry():
    """What the prepare step chose for the last call."""
    g = lib().emu_dtw_geometry()
    return dict(launches=g[13], grid=g[14], lds_bytes=g[15], fast=g[16])


def _guarded(a, poison=np.nan):
    """(raw array with poisoned bands, pointer to the payload) of an array (float32, int32 or uint8)."""
    a = np.ascontiguousarray(a).ravel()
    fill = poison if a.dtype == np.float32 else (BYTE_POISON if a.dtype == np.uint8 else -(2 ** 31))
    raw = np.full(a.size + 2 * BAND, fill, a.dtype)
    raw[BAND:BAND + a.size] = a
    return raw, raw.ctypes.data + a.dtype.itemsize * BAND


def _rows(x, pad, poison=np.nan):
    """x (B, R, T) with `pad` poisoned columns behind every row: (raw, pointer, row stride)."""
    B, R, T = x.shape
    fill = poison if x.dtype == np.float32 else BYTE_POISON
    body = np.full((B, R, T + pad), fill, x.dtype)
    body[:, :, :T] = x
    raw, ptr = _guarded(body, poison)
    return raw, ptr, T + pad


def _payload(raw, B, R, T, rs, what):
    body = raw[BAND:-BAND].reshape(B, R, rs)
    if raw.dtype == np.float32:
        clean = np.isnan(raw[:BAND]).all() and np.isnan(raw[-BAND:]).all() and np.isnan(body[:, :, T:]).all()
    else:
        clean = (raw[:BAND] == BYTE_POISON).all() and (raw[-BAND:] == BYTE_POISON).all() and (body[:, :, T:] == BYTE_POISON).all()
    assert clean, f"{what}: a band or a pad column was written"
    assert lib().emu_dtw_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"
    return body[:, :, :T].copy()


def _table(steps, add, mul):
    ab = np.ascontiguousarray(np.asarray(steps, np.int32).reshape(-1, 2))
    n = ab.shape[0]
    add = np.zeros(n, np.float32) if add is None else np.ascontiguousarray(add, np.float32)
    mul = np.ones(n, np.float32) if mul is None else np.ascontiguousarray(mul, np.float32)
    return ab, add, mul, n


DEFAULT_STEPS = ((1, 1), (0, 1), (1, 0))


def cost(X, Y, metric, *, pad_x=0, pad_y=0, pad_out=0, grid=0):
    """C (B, N, M) float32 of X (B, d, N), Y (B, d, M) through the emulated C entry; X, Y and C lie between NaN bands
    with NaN pad columns: a read outside a row puts a NaN into a sum."""
    X = np.asarray(X, np.float32)
    Y = np.asarray(Y, np.float32)
    B, d, N = X.shape
    M = Y.shape[2]
    xraw, xptr, x_rs = _rows(X, pad_x)
    yraw, yptr, y_rs = _rows(Y, pad_y)
    rs = M + pad_out
    oraw = np.full(B * N * rs + 2 * BAND, np.nan, np.float32)
    _check(lib().emu_dtw_cost_f32(xptr, yptr, B, d, N, M, x_rs, y_rs, METRICS[metric], oraw.ctypes.data + 4 * BAND, rs, int(grid)))
    got = _payload(oraw, B, N, M, rs, "C")
    assert not np.isnan(got).any(), "a value is NaN or was not written"
    return got


def accumulate(C, steps=None, add=None, mul=None, *, subseq=False, band_r=None, pad_in=0, pad_out=0, grid=0, poison=np.nan):
    """(D float32, codes uint8), both (B, N, M), of C (B, N, M) through the emulated C entry.  pad_in / pad_out:
    poisoned columns behind every row of C / of D and the codes (`poison`: NaN, or -inf, which wins every comparison
    it enters)."""
    C = np.asarray(C, np.float32)
    B, N, M = C.shape
    ab, add, mul, n = _table(DEFAULT_STEPS if steps is None else steps, add, mul)
    craw, cptr, c_rs = _rows(C, pad_in, poison)
    rs = M + pad_out
    draw = np.full(B * N * rs + 2 * BAND, np.nan, np.float32)
    sraw = np.full(B * N * rs + 2 * BAND, BYTE_POISON, np.uint8)
    _check(lib().emu_dtw_accumulate_f32(cptr, B, N, M, c_rs, n, ab.ctypes.data, add.ctypes.data, mul.ctypes.data, int(bool(subseq)),
                                        int(band_r is not None), int(band_r or 0), draw.ctypes.data + 4 * BAND, rs,
                                        sraw.ctypes.data + BAND, rs, int(grid)))
    D = _payload(draw, B, N, M, rs, "D")
    S = _payload(sraw, B, N, M, rs, "steps")
    assert not np.isnan(D).any() and not (S == BYTE_POISON).any(), "a cell is NaN or was not written"
    return D, S


def backtrack(S, steps=None, *, D=None, subseq=False, start=None, pad=0, grid=0):
    """A list of B paths ((L, 2) int32, or None where there is no path) of the codes S (B, N, M) through the emulated
    C entry.  D (B, N, M): for the subseq start (-inf behind its rows: a read there would win); start: (B) columns instead."""
    S = np.ascontiguousarray(S, np.uint8)
    B, N, M = S.shape
    ab, _, _, n = _table(DEFAULT_STEPS if steps is None else steps, None, None)
    sraw, sptr, s_rs = _rows(S, pad)
    draw, dptr, d_rs = (None, None, M) if D is None else _rows(np.asarray(D, np.float32), pad, -np.inf)
    traw, tptr = (None, None) if start is None else _guarded(np.asarray(start, np.int32))
    L = N + M - 1
    praw, pptr = _guarded(np.full(B * L * 2, -7, np.int32))
    lraw, lptr = _guarded(np.full(B, -7, np.int32))
    _check(lib().emu_dtw_backtrack_i32(dptr, sptr, tptr, B, N, M, d_rs, s_rs, n, ab.ctypes.data, int(bool(subseq)), pptr, lptr, int(grid)))
    low = -(2 ** 31)
    assert (praw[:BAND] == low).all() and (praw[-BAND:] == low).all() and (lraw[:BAND] == low).all() and (lraw[-BAND:] == low).all(), \
        "a band of the path or of the lengths was written"
    assert lib().emu_dtw_lds_overruns() == 0, "LDS beyond the bytes the host asked for was written"
    path = praw[BAND:-BAND].reshape(B, L, 2)
    lens = lraw[BAND:-BAND]
    out = []
    for b in range(B):
        n_cells = int(lens[b])
        assert n_cells == -1 or 1 <= n_cells <= L, f"pair {b}: length {n_cells}"
        assert n_cells < 0 or (path[b, n_cells:] == -7).all(), f"pair {b}: the path was written beyond its length"
        out.append(None if n_cells < 0 else path[b, :n_cells].copy())
    return out


def cost_raw(x_ptr, y_ptr, B, d, N, M, x_rs, y_rs, metric, c_ptr, c_rs):
    """The status of the prepare step for arguments that must not launch."""
    return lib().emu_dtw_cost_f32(x_ptr, y_ptr, B, d, N, M, x_rs, y_rs, metric, c_ptr, c_rs, 0)


def accumulate_raw(c_ptr, B, N, M, c_rs, steps, d_ptr, d_rs, s_ptr, s_rs, band_r=None, weights=True):
    ab = np.ascontiguousarray(np.asarray(steps, np.int32).reshape(-1, 2))
    n = ab.shape[0]
    w = np.ones(max(n, 1), np.float32)
    return lib().emu_dtw_accumulate_f32(c_ptr, B, N, M, c_rs, n, ab.ctypes.data if n else None, w.ctypes.data if weights else None,
                                        w.ctypes.data if weights else None, 0, int(band_r is not None), int(band_r or 0), d_ptr, d_rs,
                                        s_ptr, s_rs, 0)


def backtrack_raw(d_ptr, s_ptr, B, N, M, d_rs, s_rs, steps, subseq, path_ptr, len_ptr):
    ab = np.ascontiguousarray(np.asarray(steps, np.int32).reshape(-1, 2))
    return lib().emu_dtw_backtrack_i32(d_ptr, s_ptr, None, B, N, M, d_rs, s_rs, ab.shape[0], ab.ctypes.data, int(subseq), path_ptr, len_ptr, 0)
